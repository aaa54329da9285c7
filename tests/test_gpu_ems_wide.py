"""EMS decoding on codes with checks above degree 8 on a real MI355X (nbl_create_ems_wide; nbl_cn_ems_wide.hip, the programme of
nbl_cn_ems_wide_core.h) against the canonical oracle (tests/ems_wide_cases.py), flooding and layered, bit for bit.  On every code both
programmes can run -- one wave per check (nbl_cn_ems_core.h, and the specialised kernels) and one workgroup per check, selected by
nbl_debug_force_generic(dec, 3) -- they must give the same bits.  Every case is at most 9 frames of at most 88 symbols."""
import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
import ems_wide_cases as wc
import soft_ref
from conftest import load_golden, decoder_kwargs
from degree_util import profile_code, spec_edges
from test_abi import _ring_code
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def wide_decoder(name, which, iters=wc.MAX_ITER, **extra):
    code, kw, _ = wc.wide_case(name)
    dec = nb.Decoder(code, nb.METHOD_EMS, iters, layers=None if which == "flooding" else "greedy", wide=True, **kw, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, wc.layer_of(name, which))
    else:
        assert dec.layers is None
    return dec


def equal_to(dec, got, ref, tag, B):
    """out_sym, converged, iters, post and c2v of codewords 0 .. B-1 of the last decode against the reference of frame b % F: bit for bit"""
    out, conv, its = got
    for b in range(B):
        r_out, r_conv, r_its, r_post, r_c2v = ref[b % len(ref)]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, _, c2v = dec.read_state(b, v2c=False)
        assert np.array_equal(post, r_post), (tag, b, "post", float(np.max(np.abs(post - r_post))))
        assert np.array_equal(c2v, r_c2v), (tag, b, "c2v", float(np.max(np.abs(c2v - r_c2v))))


@pytest.mark.parametrize("mode", ["early-exit", "fixed"])
@pytest.mark.parametrize("which", wc.SCHEDULES)
@pytest.mark.parametrize("name", wc.NAMES)
def test_parity_with_the_canonical_oracle(oracle, name, which, mode):
    """B = 9 codewords (the frames of the case, repeated): out_sym, converged and iters equal the canonical oracle's, post and c2v equal
    its bit for bit -- under early exit (poll_every = 1) and under fixed iterations; layered: tests/layered_ref.py on the oracle's check
    node.  Check degrees 9 .. 32 over GF(4) .. GF(256) (idle lanes, one, two and four waves per check), nm = q, nm no power of two,
    nc >= dc - 1 and nc = 0, degree 2 beside degree 32 with variables of degree 1 and 8."""
    code = wc.wide_case(name)[0]
    assert code.chk_deg.max() > 8
    fixed = int(mode == "fixed")
    ref = wc.wide_reference(name, which, fixed)
    dec = wide_decoder(name, which, **(dict(fixed_iters=1) if fixed else dict(poll_every=1)))
    L = wc.batch(name)
    equal_to(dec, dec.decode(L), ref, (name, which, mode), L.shape[0])
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    if fixed:
        assert n_vn == n_syn == wc.MAX_ITER and n_cn == wc.MAX_ITER * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    dec.close()


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_batch_edges_and_the_active_list(oracle, which):
    """B = 1; a workspace that grows; and 1035 codewords under polling, where the active list takes over after the first window with
    frames leaving through early exit beside ones that stay."""
    name = "gf16-shaped"
    ref = wc.wide_reference(name, which)
    dec = wide_decoder(name, which, max_batch=1)
    equal_to(dec, dec.decode(wc.batch(name, 1)), ref, ("B1", which), 1)
    equal_to(dec, dec.decode(wc.batch(name, 3)), ref, ("B3", which), 3)
    if which == "flooding":
        assert dec.read_state(0)[1].any()                                # v2c: as on the flooding EMS decoder of nbl_create
    else:
        with pytest.raises(nb.NblError) as e:                            # refused as on the decoder of nbl_create_layered
            dec.read_state(0)
        assert e.value.status == -2 and "never materialises v2c" in str(e.value)
    dec.close()
    dec = wide_decoder(name, which, poll_every=1)
    dec.record_state(False)
    big = wc.batch(name, 1035)
    out, conv, its = dec.decode(big)
    for b in range(big.shape[0]):
        r = ref[b % len(ref)]
        assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, "active list", b)
    dec.close()


@pytest.mark.parametrize("name", ["deg_wide_gf64_ems", "deg_wide_gf16_ems", "deg_wide_gf256_ems"])
def test_wide_fixture_outputs_equal_the_compiled_reference(name):
    """The deg_wide_* fixtures: decisions, flags and iteration-count behaviour equal the compiled reference's at every recorded iteration
    count, flooding; the recorded state within the canonical tolerance of tests/test_oracle_golden.py."""
    g, meta = load_golden(name)
    code, _ = spec_edges(meta["spec"])
    kw = {k: v for k, v in decoder_kwargs(meta["profile"]).items() if k.startswith("ems_")}
    L = g["L_ch"]
    for k, it in enumerate(g["iters"]):
        dec = nb.Decoder(code, nb.METHOD_EMS, int(it), wide=True, **kw)
        out, conv, _ = dec.decode(L)
        dec.close()
        assert np.array_equal(out, g["out"][k]) and np.array_equal(conv, g["syn_ok"][k]) and np.array_equal(conv, g["ret"][k]), (name, int(it))
    for k, it in enumerate(g["state_iters"]):
        dec = nb.Decoder(code, nb.METHOD_EMS, int(it), wide=True, **kw)
        dec.record_state(True)
        dec.decode(L)
        for li, b in enumerate(int(x) for x in g["state_lanes"]):
            post, _, c2v = dec.read_state(b, v2c=False)
            for a, rf in ((post, g["st_post"][k, li]), (c2v, g["st_c2v"][k, li])):
                assert np.max(np.abs(a - rf)) <= 1e-9 * max(1.0, np.max(np.abs(rf))), (name, int(it), b)
        dec.close()


def _two_programme_case(name):
    if name == "ring256":
        return _ring_code(256, 8, 4), dict(ems_nm=32, ems_nc=3)          # the fused GF(256) kernel
    if name == "ring64":
        return _ring_code(64, 8, 4), dict(ems_nm=8, ems_nc=2, ems_factor=1.15, ems_offset=0.2)
    if name == "ring128-dc8":
        return _ring_code(128, 12, 8), dict(ems_nm=8, ems_nc=3)
    return profile_code("all", 16)[0], dict(ems_nm=6, ems_nc=2, ems_factor=1.1, ems_offset=0.1)


@pytest.mark.parametrize("which", wc.SCHEDULES)
@pytest.mark.parametrize("name", ["ring256", "ring64", "ring128-dc8", "all-16"])
def test_two_programmes_one_answer(name, which):
    """Codes with checks of degree 2 .. 8: decoded once as nbl_create / nbl_create_layered makes the decoder and once through
    nbl_create_ems_wide under nbl_debug_force_generic(dec, 3).  Outputs and the whole message state are identical."""
    code, kw = _two_programme_case(name)
    assert code.chk_deg.max() <= 8
    L = np.random.default_rng(code.q).normal(-1.5, 3.0, (4, code.N, code.q - 1))
    L[1, ::3] = 0.0                                                      # every third symbol erased
    layers = None if which == "flooding" else "greedy"
    runs = []
    for wide in (False, True):
        dec = nb.Decoder(code, nb.METHOD_EMS, 4, layers=layers, fixed_iters=1, **kw, **(dict(wide=True) if wide else {}))
        if wide:
            _force_generic(dec, 3)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        runs.append((out.copy(), conv.copy(), its.copy(), [dec.read_state(b, v2c=layers is None) for b in range(L.shape[0])]))
        if wide:
            _force_generic(dec, 0)
        dec.close()
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, which)
    assert any(s[2].any() for s in a[3]), "no check node ran"
    for f, (sa, sb) in enumerate(zip(a[3], b[3])):
        for what, x, y in zip(("post", "v2c", "c2v"), sa, sb):
            assert (x is None and y is None) or np.array_equal(x, y), (name, which, f, what)


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_wide_decoder_on_a_small_code_is_the_decoder_of_nbl_create(which):
    """Without the debug switch a wide decoder on a code with checks of degree 8 or less runs what nbl_create / nbl_create_layered runs:
    same outputs, same state, same launch counts (the fused iteration makes no variable-node launch)."""
    code, kw = _two_programme_case("ring256")
    L = np.random.default_rng(3).normal(-1.5, 3.0, (3, code.N, code.q - 1))
    layers = None if which == "flooding" else "greedy"
    runs = []
    for wide in (False, True):
        dec = nb.Decoder(code, nb.METHOD_EMS, 3, layers=layers, **kw, **(dict(wide=True) if wide else {}))
        got = dec.decode(L)
        runs.append((got, dec.last_timing()[1], [dec.read_state(b, post=False, v2c=False)[2] for b in range(3)]))
        dec.close()
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert tuple(runs[0][1]) == tuple(runs[1][1]) and (which != "flooding" or runs[0][1][0] == 0)
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_bit_llr_input_and_soft_output(which):
    """decode_bits equals decode on the expanded LLRs; the max-log symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit
    tests/soft_ref.py on this decoder's own c2v, and the bit LLRs its max-log marginals."""
    name = "gf16-shaped"
    code = wc.wide_case(name)[0]
    p = code.q.bit_length() - 1
    sigma = 0.45
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    dec = wide_decoder(name, which)
    want = dec.decode(L)
    got = dec.decode_bits(lam)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)

    class G:
        N, voff = code.N, np.concatenate([[0], np.cumsum(code.var_deg)])
    sym, bits = dec.soft_output("maxlog")
    ext, _ = dec.soft_output("maxlog", extrinsic=True)
    for b in range(4):
        c2v = dec.read_state(b, v2c=False)[2]
        assert c2v.any() or want[2][b] == 1
        P = soft_ref.posterior(L[b], c2v, G)
        assert soft_ref.bits_equal(sym[b], P), b
        assert soft_ref.bits_equal(bits[b], soft_ref.bit_marginals(P, p, soft_ref.MAXLOG)), b
        assert soft_ref.bits_equal(ext[b], soft_ref.posterior(np.zeros_like(L[b]), c2v, G)), b
    assert any(want[2][b] > 1 for b in range(4))
    dec.close()


def test_decode_samples_with_a_bpsk_demodulator(oracle):
    """nbl_decode_batch_samples on a wide decoder: the LLRs the device forms (nbl_debug_read_lch) decoded by the host entry point give the
    same outputs, and the canonical oracle gives them on those LLRs."""
    name = "gf64-nm8"
    code, kw, _ = wc.wide_case(name)
    p = code.q.bit_length() - 1
    nbits = code.N * p
    points = np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])])
    rng = np.random.default_rng(41)
    rx = np.zeros((6, nbits, 2))
    sigmas = (0.25, 0.32, 0.36, 0.4, 0.5, 0.6)
    for b, s in enumerate(sigmas):
        rx[b, :, 0] = points[0, 0] + s * rng.standard_normal(nbits)
        rx[b, :, 1] = s * rng.standard_normal(nbits)
    dec = wide_decoder(name, "flooding")
    dec.set_demodulator(2, nbits, np.arange(nbits), points)
    got, lch = [], []
    for b, s in enumerate(sigmas):                                        # (one noise level per call)
        got.append(dec.decode_samples(rx[b:b + 1], s))
        lch.append(dec.read_lch(0))
    host = [dec.decode(x[None]) for x in lch]
    dec.close()
    od, _ = wc._oracle(name, wc.MAX_ITER, 0)
    flags = []
    for b in range(len(sigmas)):
        for x, y in zip(got[b], host[b]):
            assert np.array_equal(x, y), b
        r, out, it = od.decode(lch[b])
        assert (got[b][1][0], got[b][2][0]) == (r, it) and np.array_equal(got[b][0][0], out), b
        flags.append(r)
    assert 0 < sum(flags) < len(flags), flags


def test_harness_switch(tmp_path):
    """NBL_EMS_WIDE=1 in the host layer: the harness (nbldpc_sim) on the shipped GF(16) code, EMS, BPSK at 2 dB, under NBL_SCHEDULE=flooding and
    layered.  Its checks have degree 4 and 5, so the decoder is the one nbl_create / nbl_create_layered makes and the report is the same
    with and without the switch.  A log-QSPA profile, a schedule the entry point does not have and an unknown value are refused with a
    message."""
    from nbldpc_amd import hostlib
    from test_gpu_fht import _harness
    from test_layered import GF16
    kw = dict(gfq=16, method=nb.METHOD_EMS, max_iter=10, ems_nm=8, ems_nc=2, parallel=8, crc_len=8, random_msg=1, min_sim_cycle=64, snr_begin=2.0,
              snr_step=1.0, snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    for sched in ("flooding", "layered"):
        reports = []
        for env in (dict(NBL_SCHEDULE=sched), dict(NBL_SCHEDULE=sched, NBL_EMS_WIDE="1"), dict(NBL_SCHEDULE=sched, NBL_EMS_WIDE="0")):
            rc, mean, text = _harness(str(tmp_path), env)
            assert rc == 0 and mean is not None and mean > 1.0, text
            rows = [ln.split("\t")[:7] for ln in text.splitlines() if ln.startswith("2\t")]      # the point's row without its time
            assert rows and len(rows[-1]) == 7, text                                                 # (progress rows come first)
            reports.append((mean, rows[-1]))
        assert reports[0] == reports[1] == reports[2], reports
    rc, _, text = _harness(str(tmp_path), dict(NBL_EMS_WIDE="yes"))
    assert rc != 0 and "NBL_EMS_WIDE=yes: unknown value" in text, text
    rc, _, text = _harness(str(tmp_path), dict(NBL_EMS_WIDE="1", NBL_SCHEDULE="layered-damped"))
    assert rc != 0 and "NBL_EMS_WIDE=1" in text, text
    bp = tmp_path / "bp"
    bp.mkdir()
    hostlib.prepare_workdir(str(bp), dict(kw, method=nb.METHOD_BP), GF16, "BPSK")
    rc, _, text = _harness(str(bp), dict(NBL_EMS_WIDE="1"))
    assert rc != 0 and "EMS (method 2)" in text, text
