"""T-EMS decoding on codes whose trellis path does not fit 32 bits, on a real MI355X (nbl_create_tems_wide; nbl_cn_tems_wide.hip, the
programme of nbl_cn_tems_wide_core.h with the path code of nbl_tems_path.h) against the canonical oracle (tests/tems_wide_cases.py),
flooding and damped layered, bit for bit: out_sym, converged, iters, post, c2v and v2c.  On every code both programmes can run -- one wave
per check with the 32-bit path code (nbl_cn_tems_core.h, and the specialised kernels) and one workgroup per check, selected by
nbl_debug_force_generic(dec, 3) -- they must give the same bits.  Every case is at most 9 frames of at most 88 symbols."""
import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
import tems_wide_cases as tc
import soft_ref
from conftest import load_golden, decoder_kwargs
from degree_util import TEMS_REFUSED, PROFILES, profile_code, spec_edges
from test_abi import _ring_code
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def wide_decoder(name, which, iters=tc.MAX_ITER, **extra):
    code, kw, _ = tc.wide_case(name)
    dec = nb.Decoder(code, nb.METHOD_TEMS, iters, layers=None if which == "flooding" else "greedy", tems_wide=True, **kw, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, tc.layer_of(name, which))
    else:
        assert dec.layers is None
    return dec


def equal_to(dec, got, ref, tag, B, flooding_early_exit=False):
    """out_sym, converged, iters, post, c2v and v2c of codewords 0 .. B-1 of the last decode against the reference of frame b % F: bit
    for bit.  flooding_early_exit: v2c of a codeword that converged at iteration k >= 2 is not compared -- as on every flooding decoder
    of nbl_create the variable-node pass has written the messages of iteration k by the time the syndrome is known, the reference returns
    with those of iteration k - 1 (nbl_read_state in include/nbldpc.h); under fixed iterations and under the layered schedule it is."""
    out, conv, its = got
    for b in range(B):
        r_out, r_conv, r_its, r_post, r_c2v, r_v2c = ref[b % len(ref)]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, v2c, c2v = dec.read_state(b)
        assert np.array_equal(post, r_post), (tag, b, "post", float(np.max(np.abs(post - r_post))))
        assert np.array_equal(c2v, r_c2v), (tag, b, "c2v", float(np.max(np.abs(c2v - r_c2v))))
        if not (flooding_early_exit and r_conv and r_its >= 2):
            assert np.array_equal(v2c, r_v2c), (tag, b, "v2c", float(np.max(np.abs(v2c - r_v2c))))


@pytest.mark.parametrize("mode", ["early-exit", "fixed"])
@pytest.mark.parametrize("which", tc.SCHEDULES)
@pytest.mark.parametrize("name", tc.NAMES)
def test_parity_with_the_canonical_oracle(oracle, name, which, mode):
    """B = 9 codewords (the frames of the case, repeated): out_sym, converged and iters equal the canonical oracle's, post, c2v and v2c
    equal its bit for bit -- under early exit (poll_every = 1) and under fixed iterations; layered: tests/layered_tems_ref.py on the
    oracle's check node.  Check degrees 5 .. 32 over GF(4) .. GF(256) (idle lanes, one, two and four waves per check), nr 1 .. 3,
    nc 2 .. 4, degree 2 beside degree 32 with variables of degree 1 and 8, and a code of degree <= 8 whose path needs 48 bits."""
    code, kw, _ = tc.wide_case(name)
    assert code.chk_deg.max() > 8 or (code.q.bit_length() - 1) * int(code.chk_deg.max()) > 32
    fixed = int(mode == "fixed")
    ref = tc.wide_reference(name, which, fixed)
    dec = wide_decoder(name, which, **(dict(fixed_iters=1) if fixed else dict(poll_every=1)))
    L = tc.batch(name)
    equal_to(dec, dec.decode(L), ref, (name, which, mode), L.shape[0], flooding_early_exit=which == "flooding" and not fixed)
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    if fixed:
        assert n_vn == n_syn == tc.MAX_ITER and n_cn == tc.MAX_ITER * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    dec.close()


def test_equal_costs_keep_the_first_path_in_enumeration_order(oracle):
    """Integer LLRs (tems_wide_cases.ties_frames): many paths of a check sum cost the same, and the path kept decides which symbols the
    scatter reaches.  One iteration, fixed: c2v equals the canonical oracle's bit for bit.  (tests/test_tems_wide.py shows on the CPU
    that the opposite rule gives other c2v on these frames.)"""
    code, kw, _ = tc.wide_case(tc.TIES_CASE)
    L = np.ascontiguousarray(tc.ties_frames())
    ref = tc.reference(tc.TIES_CASE, kw, L, "flooding", fixed=1, iters=1)
    dec = wide_decoder(tc.TIES_CASE, "flooding", iters=1, fixed_iters=1)
    dec.decode(L)
    for b in range(L.shape[0]):
        c2v = dec.read_state(b)[2]
        assert ref[b][4].any() and np.array_equal(c2v, ref[b][4]), (b, float(np.max(np.abs(c2v - ref[b][4]))))
    dec.close()


@pytest.mark.parametrize("which", tc.SCHEDULES)
def test_batch_edges_and_the_active_list(oracle, which):
    """B = 1; a workspace that grows; and 1035 codewords under polling, where the active list takes over after the first window with
    frames leaving through early exit beside ones that stay."""
    name = "gf16-shaped"
    ref = tc.wide_reference(name, which)
    dec = wide_decoder(name, which, max_batch=1)
    equal_to(dec, dec.decode(tc.batch(name, 1)), ref, ("B1", which), 1, flooding_early_exit=which == "flooding")
    equal_to(dec, dec.decode(tc.batch(name, 3)), ref, ("B3", which), 3, flooding_early_exit=which == "flooding")
    dec.close()
    dec = wide_decoder(name, which, poll_every=1)
    dec.record_state(False)
    big = tc.batch(name, 1035)
    out, conv, its = dec.decode(big)
    for b in range(big.shape[0]):
        r = ref[b % len(ref)]
        assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, "active list", b)
    dec.close()


@pytest.mark.parametrize("name", ["deg_wide_gf64_tems", "deg_wide_gf16_tems", "deg_wide_gf256_tems"])
def test_wide_fixture_outputs_equal_the_compiled_reference(name):
    """The deg_wide_*_tems fixtures: decisions and flags equal the compiled reference's at every recorded iteration count, flooding; the
    recorded state within the canonical tolerance of tests/test_oracle_golden.py."""
    g, meta = load_golden(name)
    code, _ = spec_edges(meta["spec"])
    kw = {k: v for k, v in decoder_kwargs(meta["profile"]).items() if k.startswith("tems_")}
    L = g["L_ch"]
    for k, it in enumerate(g["iters"]):
        dec = nb.Decoder(code, nb.METHOD_TEMS, int(it), tems_wide=True, **kw)
        out, conv, _ = dec.decode(L)
        dec.close()
        assert np.array_equal(out, g["out"][k]) and np.array_equal(conv, g["syn_ok"][k]) and np.array_equal(conv, g["ret"][k]), (name, int(it))
    for k, it in enumerate(g["state_iters"]):
        dec = nb.Decoder(code, nb.METHOD_TEMS, int(it), tems_wide=True, **kw)
        dec.record_state(True)
        dec.decode(L)
        for li, b in enumerate(int(x) for x in g["state_lanes"]):
            post, v2c, c2v = dec.read_state(b)
            for a, rf in ((post, g["st_post"][k, li]), (v2c, g["st_v2c"][k, li]), (c2v, g["st_c2v"][k, li])):
                assert np.max(np.abs(a - rf)) <= 1e-9 * max(1.0, np.max(np.abs(rf))), (name, int(it), b)
        dec.close()


def _two_programme_case(name):
    if name == "ring256":
        return _ring_code(256, 8, 4), dict(tems_nr=2, tems_nc=3)         # tems256
    if name == "ring64":
        return _ring_code(64, 8, 4), dict(tems_nr=2, tems_nc=3, tems_factor=1.15, tems_offset=0.2)       # the fused tems64
    if name == "ring16":
        return _ring_code(16, 8, 4), dict(tems_nr=2, tems_nc=4)          # nc 4: the general programme's general path
    return profile_code("all", 16)[0], dict(tems_nr=3, tems_nc=2, tems_factor=1.1, tems_offset=0.1)


@pytest.mark.parametrize("which", tc.SCHEDULES)
@pytest.mark.parametrize("name", ["ring256", "ring64", "ring16", "all-16"])
def test_two_programmes_one_answer(name, which):
    """Codes inside nbl_create's envelope: decoded once as nbl_create / nbl_create_layered_ex makes the decoder and once through
    nbl_create_tems_wide under nbl_debug_force_generic(dec, 3).  Outputs and the whole message state are identical."""
    code, kw = _two_programme_case(name)
    assert (code.q.bit_length() - 1) * int(code.chk_deg.max()) <= 32
    L = np.random.default_rng(code.q).normal(-1.5, 3.0, (4, code.N, code.q - 1))
    L[1, ::3] = 0.0                                                      # every third symbol erased
    layers = None if which == "flooding" else "greedy"
    runs = []
    for wide in (False, True):
        extra = dict(tems_wide=True) if wide else (dict(damped=True) if layers else {})
        dec = nb.Decoder(code, nb.METHOD_TEMS, 4, layers=layers, fixed_iters=1, **kw, **extra)
        if wide:
            _force_generic(dec, 3)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        runs.append((out.copy(), conv.copy(), its.copy(), [dec.read_state(b) for b in range(L.shape[0])]))
        if wide:
            _force_generic(dec, 0)
        dec.close()
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, which)
    assert any(s[2].any() for s in a[3]), "no check node ran"
    for f, (sa, sb) in enumerate(zip(a[3], b[3])):
        for what, x, y in zip(("post", "v2c", "c2v"), sa, sb):
            assert np.array_equal(x, y), (name, which, f, what)


@pytest.mark.parametrize("which", tc.SCHEDULES)
def test_wide_decoder_on_a_small_code_is_the_decoder_of_nbl_create(which):
    """Without the debug switch a wide decoder on a code inside nbl_create's envelope runs what nbl_create / nbl_create_layered_ex runs:
    same outputs, same state, same launch counts (the fused iteration makes no variable-node launch)."""
    code, kw = _two_programme_case("ring64")
    L = np.random.default_rng(3).normal(-1.5, 3.0, (3, code.N, code.q - 1))
    layers = None if which == "flooding" else "greedy"
    runs = []
    for wide in (False, True):
        extra = dict(tems_wide=True) if wide else (dict(damped=True) if layers else {})
        dec = nb.Decoder(code, nb.METHOD_TEMS, 3, layers=layers, **kw, **extra)
        got = dec.decode(L)
        runs.append((got, dec.last_timing()[1], [dec.read_state(b, post=False)[1:] for b in range(3)]))
        dec.close()
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert tuple(runs[0][1]) == tuple(runs[1][1]) and (which != "flooding" or runs[0][1][0] == 0)
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


REFUSED_CELLS = list(TEMS_REFUSED) + [("dv48", 128), ("dv48", 256)]


@pytest.mark.parametrize("prof,q", REFUSED_CELLS)
def test_cells_nbl_create_refuses_run_and_equal_the_oracle(oracle, prof, q):
    """Every (profile, q) cell of tests/degree_util.py whose T-EMS decoder nbl_create refuses for its path code (TEMS_REFUSED), and the
    dv48 cells at GF(128) / GF(256) with their full check degrees (4, 5): nbl_create still refuses, nbl_create_tems_wide decodes, and
    outputs and state equal the canonical oracle's bit for bit (flooding, 2 iterations, nr 2, nc 2)."""
    code = profile_code(prof, q)[0]                                      # (method=None: the profile's own check degrees)
    assert sorted(set(code.chk_deg.tolist())) == sorted(PROFILES[prof][0]) and (q.bit_length() - 1) * int(code.chk_deg.max()) > 32
    kw = dict(tems_nr=2, tems_nc=2)
    with pytest.raises(nb.NblError) as e:
        nb.Decoder(code, nb.METHOD_TEMS, 2, **kw)
    assert e.value.status == -2 and "32-bit" in str(e.value)
    # all-zero-codeword BPSK LLRs at noise levels of their own (the dv48 graphs have N < M: no rate to derive a level from)
    p, rng = q.bit_length() - 1, np.random.default_rng(q)
    mask = ((np.arange(1, q)[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64)
    L = np.ascontiguousarray([(-2.0 * (1.0 + s * rng.standard_normal((code.N, p))) / s ** 2) @ mask.T for s in (0.45, 0.8)])
    assert np.all(np.isfinite(L))
    ref = tc.reference(code, kw, L, "flooding", fixed=1, iters=2)
    dec = nb.Decoder(code, nb.METHOD_TEMS, 2, fixed_iters=1, tems_wide=True, **kw)
    dec.record_state(True)
    equal_to(dec, dec.decode(L), ref, (prof, q), L.shape[0])
    assert all(r[4].any() and np.all(np.isfinite(r[3])) for r in ref)
    dec.close()


@pytest.mark.parametrize("which", tc.SCHEDULES)
def test_bit_llr_input_and_soft_output(which):
    """decode_bits equals decode on the expanded LLRs; the max-log symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit
    tests/soft_ref.py on this decoder's own c2v, and the bit LLRs its max-log marginals."""
    name = "gf16-shaped"
    code = tc.wide_case(name)[0]
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
        c2v = dec.read_state(b)[2]
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
    name = "gf64-nc2"
    code, kw, _ = tc.wide_case(name)
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
    od, _ = tc.oracle_decoder(name, tc.MAX_ITER, 0, tuple(sorted(kw.items())))
    flags = []
    for b in range(len(sigmas)):
        for x, y in zip(got[b], host[b]):
            assert np.array_equal(x, y), b
        r, out, it = od.decode(lch[b])
        assert (got[b][1][0], got[b][2][0]) == (r, it) and np.array_equal(got[b][0][0], out), b
        flags.append(r)
    assert 0 < sum(flags) < len(flags), flags


def test_harness_switch(tmp_path):
    """NBL_TEMS_WIDE=1 in the host layer: the harness (nbldpc_sim) on the shipped GF(16) code, T-EMS, BPSK at 2 dB, under
    NBL_SCHEDULE=flooding and layered-damped.  Its checks have degree 4 and 5 (20 bits of path), so the decoder is the one nbl_create /
    nbl_create_layered_ex makes and the report is the same with and without the switch.  An EMS profile, a schedule the entry point does
    not have and an unknown value are refused with a message."""
    from nbldpc_amd import hostlib
    from test_gpu_fht import _harness
    from test_layered import GF16
    kw = dict(gfq=16, method=nb.METHOD_TEMS, max_iter=10, tems_nr=2, tems_nc=3, parallel=8, crc_len=8, random_msg=1, min_sim_cycle=64, snr_begin=2.0,
              snr_step=1.0, snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    for sched in ("flooding", "layered-damped"):
        reports = []
        for env in (dict(NBL_SCHEDULE=sched), dict(NBL_SCHEDULE=sched, NBL_TEMS_WIDE="1"), dict(NBL_SCHEDULE=sched, NBL_TEMS_WIDE="0")):
            rc, mean, text = _harness(str(tmp_path), env)
            assert rc == 0 and mean is not None and mean > 1.0, text
            rows = [ln.split("\t")[:7] for ln in text.splitlines() if ln.startswith("2\t")]      # the point's row without its time
            assert rows and len(rows[-1]) == 7, text                                                 # (progress rows come first)
            reports.append((mean, rows[-1]))
        assert reports[0] == reports[1] == reports[2], reports
    rc, _, text = _harness(str(tmp_path), dict(NBL_TEMS_WIDE="yes"))
    assert rc != 0 and "NBL_TEMS_WIDE=yes: unknown value" in text, text
    rc, _, text = _harness(str(tmp_path), dict(NBL_TEMS_WIDE="1", NBL_SCHEDULE="layered"))
    assert rc != 0 and "NBL_TEMS_WIDE=1" in text, text
    ems = tmp_path / "ems"
    ems.mkdir()
    hostlib.prepare_workdir(str(ems), dict(kw, method=nb.METHOD_EMS), GF16, "BPSK")
    rc, _, text = _harness(str(ems), dict(NBL_TEMS_WIDE="1"))
    assert rc != 0 and "T-EMS (method 4)" in text, text
