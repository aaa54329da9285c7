"""The synthetic OSD shapes of tests/osd_shapes.py: the properties their table states, the full-rank condition computed in Python
against nbl_create_osd's own check, and the checker's counters.  No GPU."""
import numpy as np
import pytest

import nbldpc_amd as nb
import osd_shapes as sh
from osd_util import build_checker, run_checker


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("osd"))


def _create(code, name, **kw):
    crc_len, crc_rows = sh.crc_of(name)
    return nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=4, ems_nc=2, osd_order=2, osd_flag=1, crc_len=crc_len, crc_rows=crc_rows, **kw)


def test_table_holds_the_issue_shapes():
    want = {"one_word", "just_over_64", "gf8_odd", "gf8_trunc", "gf128", "trunc_on_boundary", "just_over_512", "cap", "below_cap",
            "high_rate", "low_rate", "k1", "k2", "irregular"} | set(sh.CRC_PARTIAL)
    assert want <= set(sh.SHAPES)
    assert {sh.SHAPES[s]["q"] for s in sh.SHAPES} >= {4, 8, 16, 32, 128}
    assert sh.lds_bytes(1024) == sh.CAP_LDS and sh.lds_bytes(576) == 67000
    # the distance length falls on a word boundary below n for one (N, q) only
    assert [(N, q) for q in (4, 8, 16, 32, 64, 128, 256) for N in range(1, 1024 // (q.bit_length() - 1) + 1)
            if sh.n_dist(N, q) < N * (q.bit_length() - 1) and sh.n_dist(N, q) % 64 == 0] == [(299, 8)]


@pytest.mark.parametrize("name", sorted(sh.SHAPES))
def test_shape_has_its_property_and_passes_creation(name):
    """shape() asserts the stated property and the Python rank; nbl_create_osd then fails, if at all, only for want of a device."""
    import torch
    code, _, _, info = sh.shape(name)
    if name == "high_rate":
        assert info["k"] >= 7 * info["R"]
    if name == "low_rate":
        assert info["R"] >= 7 * info["k"]
    if name in sh.CRC_PARTIAL:
        assert 0 < info["crc_rows"] < info["crc_len"]
    if name in sh.TRUNCATED:
        assert info["n_dist"] == info["n"] - 1
    if name == "just_over_512":
        assert sh.zero_block_variables(code), "the rotation at num_temp = 512 needs an all-zero column"
    try:
        d = _create(code, name)
        assert torch.cuda.is_available()
        d.close()
    except nb.NblError as e:
        assert e.status == -3 and not torch.cuda.is_available(), (name, str(e))


BAD = sorted(s for s in sh.SHAPES if sh.SHAPES[s]["bad_seed"] is not None)


@pytest.mark.parametrize("name", BAD)
def test_seed_the_python_rank_rejects_is_refused(name):
    assert len(BAD) >= 5
    code, _, _ = sh.build(name, sh.SHAPES[name]["bad_seed"])
    crc_len, crc_rows = sh.crc_of(name)
    assert not sh.full_rank(code, crc_len, crc_rows)
    with pytest.raises(nb.NblError) as e:
        _create(code, name)
    assert e.value.status == -2 and "full row rank" in str(e.value), str(e.value)


def test_full_set_of_gf_matrices_changes_the_rank_input():
    """The zero block of alpha^(q-2) is part of the matrix: with the full set of element matrices the same graph has other rows."""
    code, _, _, _ = sh.shape("just_over_512")
    full = nb.datafiles.gf_matrices(8, as_loaded=False)
    assert not np.array_equal(sh.osd_matrix(code), sh.osd_matrix(code, gf_mat=full))
    v = sh.zero_block_variables(code)[0]
    assert not sh.osd_matrix(code)[:, 3 * v:3 * v + 3].any()


def test_counters_do_not_change_the_output_and_count(checker):
    """The third argument of the checker: same decisions with and without it; a frame whose least reliable bit sits in an all-zero
    column rotates at num_temp = n - 1, and a frame scaled beyond 1,000,000 keeps the base word (-1 flips)."""
    code, _, _, info = sh.shape("just_over_512")
    rng = np.random.default_rng(3)
    L = sh.bpsk_llr_zero(rng, code, 3, 1.0)
    L[1, sh.zero_block_variables(code)[0]] *= 1e-3
    L[2] *= 1e6
    out = run_checker(checker, code, L, 1)
    out2, c = run_checker(checker, code, L, 1, counters=True)
    assert np.array_equal(out, out2)
    assert c["max_rot"][1] == info["n"] - 1 and c["rotations"][1] >= 1
    assert c["flips"][2] == -1 and c["differs"][2] == 0 and c["best"][2] >= 1e6
    assert (c["flips"][:2] >= 0).all() and (c["best"][:2] < 1e6).all()


@pytest.mark.parametrize("name", sorted(sh.SHAPES))
def test_coverage_conditions_hold_on_the_cpu(oracle, checker, name):
    """What tests/test_gpu_osd_shapes.py asserts about its own inputs, from the checker's counters and the oracle's flags alone: the
    seeds and noise levels were chosen here, without a GPU."""
    c = sh.case(name, checker)
    sh.assert_coverage(name, c)
    q = c["code"].q
    for iters in (1, 2):
        od = oracle.Decoder(oracle.Code(edges=c["edges"]), oracle.GF(q), oracle.EMS, iters, oracle.CANONICAL, ems_nm=min(q, 6), ems_nc=2)
        flags = [od.decode(L)[0] for L in c["L"]]
        assert 0 < sum(flags) < len(flags), (name, iters, flags)
