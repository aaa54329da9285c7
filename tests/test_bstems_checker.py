"""Basic-set T-EMS (decode method 7), CPU side: the checker tests/bstems_check.cpp in LITERAL mode reproduces every bstems_*.npz
(dumped from the compiled reference) bit for bit, and the C ABI takes the method through nbl_create_ex.  No GPU involved."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from conftest import GOLD, load_golden
from bstems_util import LITERAL, CANONICAL, bs_kwargs, build_checker, ring_code, run_checker

SETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "bstems_*.npz")))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bstems"))


def test_fixture_sets_present():
    assert len(SETS) >= 6, SETS
    for name in SETS:
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 1 << 20, name


@pytest.mark.parametrize("name", SETS)
def test_literal_checker_equals_reference(checker, name):
    g, meta = load_golden(name)
    p = meta["profile"]
    assert p["method"] == 7
    code = nb.Code(meta["code"])
    L = g["L_ch"]
    kw = bs_kwargs(p)
    for k, it in enumerate(g["iters"]):
        out, ret, its, _ = run_checker(checker, code, L, int(it), LITERAL, kw["bs_nm"], kw["bs_nc"], kw["bs_factor"], kw["bs_offset"])
        assert np.array_equal(out, g["out"][k]), (name, it)
        assert np.array_equal(ret, g["ret"][k]), (name, it)
    lanes = [int(b) for b in g["state_lanes"]]
    for k, it in enumerate(g["state_iters"]):
        _, _, _, st = run_checker(checker, code, L[:max(lanes) + 1], int(it), LITERAL, kw["bs_nm"], kw["bs_nc"], kw["bs_factor"],
                                  kw["bs_offset"], state=lanes)
        for j, b in enumerate(lanes):
            post, v2c, c2v = st[b]
            assert np.array_equal(post, g["st_post"][k][j]), (name, it, b, "post")
            assert np.array_equal(v2c, g["st_v2c"][k][j]), (name, it, b, "v2c")
            assert np.array_equal(c2v, g["st_c2v"][k][j]), (name, it, b, "c2v")


def test_canonical_checker_agrees_on_decisions(checker):
    """CANONICAL differs from LITERAL only by the running-sum residue of the configuration costs (and the tie rule of the symbol
    order): on the fixtures the decisions, flags and iteration counts are the same."""
    for name in SETS:
        g, meta = load_golden(name)
        kw = bs_kwargs(meta["profile"])
        code = nb.Code(meta["code"])
        it = int(g["iters"][-1])
        a = run_checker(checker, code, g["L_ch"], it, LITERAL, **kw)
        b = run_checker(checker, code, g["L_ch"], it, CANONICAL, **kw)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x, y), name


def test_checker_fixed_iterations_freeze_outputs(checker):
    """fixed_iters = 1 runs every codeword max_iter iterations; outputs, flags and iteration counts are those of the early exit."""
    g, meta = load_golden("bstems_gf16_u128")
    kw = bs_kwargs(meta["profile"])
    code = nb.Code(meta["code"])
    a = run_checker(checker, code, g["L_ch"], 20, CANONICAL, **kw)
    b = run_checker(checker, code, g["L_ch"], 20, CANONICAL, fixed_iters=1, **kw)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert (a[1] == 1).any() and (a[2] < 20).any()


def test_checker_runs_the_synthetic_grid(checker):
    """Every (q, nm, nc) of the GPU grid test runs on the checker (q = 4 with nm = 3 = q - 1 > p included)."""
    rng = np.random.default_rng(5)
    for q in (4, 8, 32, 128):
        code = ring_code(q, 8, 4)
        L = rng.normal(0.0, 2.0, size=(2, code.N, q - 1))
        for nm in sorted({1, min(q - 1, 16)} | {n for n in (2, 3, 5, 7, 12) if n < q}):
            for nc in range(0, 5):
                out, ret, its, _ = run_checker(checker, code, L, 3, CANONICAL, nm, nc)
                assert out.shape == (2, code.N) and (its <= 3).all()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------

def _create_ex(code, bs_nm, bs_nc=2, bs_factor=1.0, bs_offset=0.0, method=7):
    return nb.Decoder(code, method=method, max_iter=5, bs_nm=bs_nm, bs_nc=bs_nc, bs_factor=bs_factor, bs_offset=bs_offset)


def test_create_ex_is_declared_and_exported():
    lib = nb.load_library()
    assert hasattr(lib, "nbl_create_ex")
    assert "nbl_create_ex" in nb.EXPORTS
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "nbldpc.h")).read()
    assert "nbl_create_ex(" in hdr and "NBL_METHOD_BS_TEMS 7" in hdr and "nbl_params_ext" in hdr
    assert nb.METHOD_BS_TEMS == 7
    assert lib.nbl_abi_version() == 1


def test_create_ex_accepts_bstems_parameters():
    """Valid BS-TEMS parameters get past every check: without a GPU the call ends at the device query (-3), with one it succeeds."""
    import torch
    for q, nm, nc in ((16, 4, 2), (16, 15, 4), (256, 8, 3), (256, 16, 4), (4, 3, 0)):
        code = ring_code(q, 8, 4) if q != 16 else nb.Code("divsalar.UNBLDPC.128.64.GF.16")
        if torch.cuda.is_available():
            _create_ex(code, nm, nc).close()
            continue
        with pytest.raises(nb.NblError) as e:
            _create_ex(code, nm, nc)
        assert e.value.status == -3, (q, nm, nc, str(e.value))


def test_create_ex_rejects_bad_bstems_parameters():
    code = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    cases = [(dict(bs_nm=16), -1, "bs_nm"),          # nm >= q: the reference reads past its basic-set arrays
             (dict(bs_nm=0), -1, "bs_nm"),
             (dict(bs_nm=4, bs_nc=-1), -1, "bs_nc"),
             (dict(bs_nm=4, bs_factor=0.0), -1, "bs_factor")]
    for kw, status, word in cases:
        with pytest.raises(nb.NblError) as e:
            _create_ex(code, **kw)
        assert e.value.status == status and word in str(e.value), (kw, str(e.value))
    big = ring_code(256, 8, 4)
    with pytest.raises(nb.NblError) as e:
        _create_ex(big, bs_nm=17)                     # above the kernel's cap of 16 elements
    assert e.value.status == -2 and "16" in str(e.value)


def test_create_without_ext_still_refuses_method_7():
    code = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    with pytest.raises(nb.NblError) as e:
        nb.Decoder(code, method=7, max_iter=5)
    assert e.value.status == -2 and "nbl_create_ex" in str(e.value)


def test_create_ex_with_null_ext_is_nbl_create():
    """nbl_create_ex(..., NULL, ...) behaves as nbl_create: method 7 is refused, the other methods get past validation."""
    import torch
    lib = nb.load_library()
    code = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    mul, inv = nb.datafiles.gf_tables(16)
    mul = np.ascontiguousarray(np.array(mul, dtype=np.uint16))
    inv = np.ascontiguousarray(np.array(inv, dtype=np.uint16))
    desc = code.desc()
    h = C.c_void_p()
    prm = nb.binding.Params(7, 5, 8, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    rc = lib.nbl_create_ex(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None, 0, C.byref(h))
    assert rc == -2 and not h.value
    prm = nb.binding.Params(2, 5, 8, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    rc = lib.nbl_create_ex(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None, 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0
        lib.nbl_destroy(h)
    else:
        assert rc == -3
