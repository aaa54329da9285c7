"""Min-Max decoding (method 3, nbl_create_minmax; nbl_cn_minmax.hip, the programme of nbl_cn_minmax_core.h) on a real MI355X against the
numpy restatement of include/nbldpc.h (tests/minmax_ref.py, cases of tests/minmax_cases.py), flooding and layered.  The method is defined
by set -- between its two rounded subtractions there is only min and max -- so every comparison is np.array_equal: out_sym, converged,
iters, post and c2v.  Every case is at most 9 frames of at most 88 symbols."""
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
import minmax_cases as mc
import minmax_ref as mr
import soft_ref
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def decoder(name, which, iters=mc.MAX_ITER, **extra):
    code, kw, _ = mc.case(name)
    layers = None if which == "flooding" else "greedy" if which == "greedy" else mc.layer_of(name, which)
    dec = nb.Decoder(code, nb.METHOD_MINMAX, iters, layers=layers, minmax=True, **kw, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, mc.layer_of(name, which))
    else:
        assert dec.layers is None                                         # nbl_get_layers is NBL_ERR_ARG on the flooding kind
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
@pytest.mark.parametrize("which", mc.SCHEDULES)
@pytest.mark.parametrize("name", mc.NAMES)
def test_parity_with_the_restatement(name, which, mode):
    """B = 9 codewords (the frames of the case, repeated) under early exit (poll_every = 1) and under fixed iterations.  GF(4) .. GF(256):
    idle lanes, one, two and four waves per check; degree 2 beside degree 32 with variables of degree 1 and 8; shaping; the shipped
    codes' shape.  The debug switch changes nothing: there is one programme."""
    fixed = int(mode == "fixed")
    ref = mc.reference(name, which, fixed)
    dec = decoder(name, which, **(dict(fixed_iters=1) if fixed else dict(poll_every=1)))
    L = mc.batch(name)
    equal_to(dec, dec.decode(L), ref, (name, which, mode), L.shape[0])
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    if fixed:
        assert n_vn == n_syn == mc.MAX_ITER and n_cn == mc.MAX_ITER * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    if name == "mix128":
        _force_generic(dec, 3)
        again = dec.decode(L)
        _force_generic(dec, 0)
        equal_to(dec, again, ref, (name, which, mode, "switch 3"), L.shape[0])
    dec.close()


def test_one_check_per_layer():
    """an explicit assignment, the serial-C schedule: layer m holds check m alone"""
    name = "wide16"
    ref = mc.reference(name, "serial")
    dec = decoder(name, "serial", poll_every=1)
    assert int(dec.layers.max()) + 1 == mc.case(name)[0].M
    L = mc.batch(name)
    equal_to(dec, dec.decode(L), ref, (name, "serial"), L.shape[0])
    assert any(not np.array_equal(a[4], b[4]) for a, b in zip(ref, mc.reference(name, "greedy")))
    dec.close()


@pytest.mark.parametrize("which", mc.SCHEDULES)
def test_batch_sizes_1_to_17(which):
    """a workspace that grows from one codeword; every batch size up to 17"""
    name = "wide16"
    ref = mc.reference(name, which)
    dec = decoder(name, which, max_batch=1)
    dec.record_state(False)
    for B in range(1, 18):
        out, conv, its = dec.decode(mc.batch(name, B))
        for b in range(B):
            r = ref[b % len(ref)]
            assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, B, b)
    dec.record_state(True)
    equal_to(dec, dec.decode(mc.batch(name, 17)), ref, (which, "B17"), 17)
    dec.close()


@pytest.mark.parametrize("poll_every", [1, 2])
@pytest.mark.parametrize("which", mc.SCHEDULES)
def test_the_active_list(which, poll_every):
    """1035 codewords under polling: the active list takes over after the first window, with frames that leave at iteration 1 and 2
    beside ones that stay, so that slots lie beyond the list"""
    name = "wide16"
    ref = mc.reference(name, which)
    assert {r[2] for r in ref if r[1]} >= {1, 2} and any(not r[1] for r in ref)
    dec = decoder(name, which, poll_every=poll_every)
    dec.record_state(False)
    big = mc.batch(name, 1035)
    out, conv, its = dec.decode(big)
    for b in range(big.shape[0]):
        r = ref[b % len(ref)]
        assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, poll_every, "active list", b)
    dec.close()


@pytest.mark.parametrize("which", mc.SCHEDULES)
def test_read_state_refuses_v2c(which):
    name = "shaped16"
    dec = decoder(name, which)
    dec.decode(mc.batch(name, 2))
    with pytest.raises(nb.NblError) as e:
        dec.read_state(0)
    assert e.value.status == -2 and "v2c" in str(e.value)
    post, none, c2v = dec.read_state(1, v2c=False)
    assert none is None and post.any() and c2v.any()
    dec.record_state(False)
    dec.decode(mc.batch(name, 2))
    assert dec.read_state(1, post=False, v2c=False)[2].any()
    dec.close()


@pytest.mark.parametrize("which", mc.SCHEDULES)
def test_bit_llr_input_and_soft_output(which):
    """decode_bits equals decode on the expanded LLRs and the restatement on them; the max-log symbol LLRs of nbl_soft_output, plain and
    extrinsic, are bit for bit L_ch + the restatement's c2v in the variable's edge order, the bit LLRs its max-log marginals; the
    log-sum bit LLRs within the tolerance tests/soft_ref.py records."""
    name = "shaped16"
    code = mc.case(name)[0]
    p = code.q.bit_length() - 1
    sigma = 0.45
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    dec = decoder(name, which)
    want = dec.decode(L)
    got = dec.decode_bits(lam)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    lay = mc.layer_of(name, which)
    ref = [mr.decode(mc.checker(name), L[b], lay, mc.MAX_ITER) for b in range(4)]

    class G:
        N, voff = code.N, np.concatenate([[0], np.cumsum(code.var_deg)])
    sym, bits = dec.soft_output("maxlog")
    ext, _ = dec.soft_output("maxlog", extrinsic=True)
    _, logsum = dec.soft_output("logsum", sym=False)
    for b in range(4):
        r_out, r_conv, r_its, _, r_c2v = ref[b]
        assert (want[1][b], want[2][b]) == (r_conv, r_its) and np.array_equal(want[0][b], r_out), b
        assert np.array_equal(dec.read_state(b, v2c=False)[2], r_c2v), b
        P = soft_ref.posterior(L[b], r_c2v, G)
        assert soft_ref.bits_equal(sym[b], P), b
        assert soft_ref.bits_equal(bits[b], soft_ref.bit_marginals(P, p, soft_ref.MAXLOG)), b
        assert soft_ref.bits_equal(ext[b], soft_ref.posterior(np.zeros_like(L[b]), r_c2v, G)), b
        assert soft_ref.logsum_error(logsum[b], soft_ref.bit_marginals(P, p, soft_ref.LOGSUM), P) <= soft_ref.LOGSUM_TOL, b
    assert any(want[2][b] > 1 for b in range(4))
    dec.close()


def test_decode_samples_with_a_bpsk_demodulator():
    """nbl_decode_batch_samples on a Min-Max decoder: the LLRs the device forms (nbl_debug_read_lch) decoded by the host entry point give
    the same outputs, and the restatement gives them on those LLRs."""
    name = "wide64"
    code = mc.case(name)[0]
    p = code.q.bit_length() - 1
    nbits = code.N * p
    points = np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])])
    rng = np.random.default_rng(41)
    sigmas = (0.25, 0.32, 0.36, 0.4, 0.5, 0.6)
    rx = np.zeros((len(sigmas), nbits, 2))
    for b, s in enumerate(sigmas):
        rx[b, :, 0] = points[0, 0] + s * rng.standard_normal(nbits)
        rx[b, :, 1] = s * rng.standard_normal(nbits)
    dec = decoder(name, "flooding")
    dec.set_demodulator(2, nbits, np.arange(nbits), points)
    got, lch = [], []
    for b, s in enumerate(sigmas):                                        # (one noise level per call)
        got.append(dec.decode_samples(rx[b:b + 1], s))
        lch.append(dec.read_lch(0))
    host = [dec.decode(x[None]) for x in lch]
    dec.close()
    flags = []
    for b in range(len(sigmas)):
        for x, y in zip(got[b], host[b]):
            assert np.array_equal(x, y), b
        out, r, it, _, _ = mr.decode(mc.checker(name), lch[b], None, mc.MAX_ITER)
        assert (got[b][1][0], got[b][2][0]) == (r, it) and np.array_equal(got[b][0][0], out), b
        flags.append(r)
    assert 0 < sum(flags) < len(flags), flags


# ---- the iterative-demapping loop -------------------------------------------------------------------------------------------------------
IDD_CELLS = {"flooding": 0.4, "greedy": 0.6}      # sigma per schedule, chosen on the restatement alone: pass 1 / later / never = (14, 4, 6), (19, 1, 4)
IDD_PASSES, IDD_ITERS, IDD_B = 3, 3, 24


@functools.lru_cache(maxsize=None)
def _idd_shape():
    import demod_general as dg
    import idd_kinds_cases as kc
    code = dg.graph("gf64_16qam_interleaved")[0]                          # GF(64) on bit-interleaved Gray 16-QAM: foreign label bits, N = 14
    return code, kc.shape("dc2mix64"), mr.MinMax(code, np.array(nb.datafiles.gf_tables(code.q)[0]))


@pytest.mark.parametrize("which", sorted(IDD_CELLS))
def test_the_loop_is_the_chain_of_public_calls_and_the_reference_loop(which):
    """nbl_decode_batch_samples_idd on a Min-Max decoder equals decode_samples, extrinsic soft output, decode_samples with that prior on
    the unconverged rows; and idd_ref.loop around the restatement, bit for bit.  Frames converge in pass 1, in a later pass and never."""
    import demod_general as dg
    import idd_kinds_cases as kc
    import idd_ref as ir
    from test_gpu_idd import same
    from test_gpu_idd_kinds import chain
    code, sh, mm = _idd_shape()
    sigma = IDD_CELLS[which]
    lay = None if which == "flooding" else nb.layer_greedy(code)

    def ref_decode(L):
        out, r, n, _, c2v = mr.decode(mm, L, lay, IDD_ITERS)
        return int(r), out, int(n), c2v
    rx = ir.loop_samples(sh, sigma, IDD_B)
    ref = ir.loop(ref_decode, mm.g, sh, rx, sigma, ir.MAXLOG, IDD_PASSES, ir.MAXLOG)
    cnt = kc.counts(ref[1], ref[3])
    print(f"minmax {which}: pass 1 / later / never = {cnt}")
    assert kc.full_mix(cnt), (which, cnt)
    for poll_every in (0, 2):
        dec = nb.Decoder(code, nb.METHOD_MINMAX, IDD_ITERS, poll_every=poll_every, layers=None if lay is None else "greedy", minmax=True)
        dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
        want = chain(dec, rx, sigma, IDD_PASSES)
        got = dec.decode_samples_idd(rx, sigma, IDD_PASSES, "maxlog")
        same(got, want, ("minmax", which, poll_every, "chain"))
        same(got, ref, ("minmax", which, poll_every, "reference"))
        dec.close()


# ---- the harness ------------------------------------------------------------------------------------------------------------------------
def test_harness_runs_a_method_3_profile(tmp_path, monkeypatch):
    """A profile with DecodeMethod = 3 in the host layer: the harness (nbldpc_sim) on the shipped GF(16) code, BPSK at 2 dB, 8 lanes, under
    NBL_SCHEDULE=flooding and layered.  Its counts are those of the same frames decoded by Decoder(minmax=True) and counted by the host
    chain's ErrCount, its iterations per frame their mean; the words the Python call decodes are the restatement's.  OSD, and a
    schedule the kind does not have, are refused with a message."""
    from nbldpc_amd import hostlib
    from test_gpu_fht import _harness
    from test_layered import GF16
    code = nb.Code(GF16)
    N, K, P = code.N, code.N - code.M, 8
    shaping = dict(ems_factor=1.1, ems_offset=0.1)
    kw = dict(gfq=16, method=nb.METHOD_MINMAX, max_iter=10, parallel=P, crc_len=8, random_msg=1, min_sim_cycle=64, snr_begin=2.0, snr_step=1.0,
              snr_stop=2.0, **shaping)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    mm = mr.MinMax(code, np.array(nb.datafiles.gf_tables(16)[0]), shaping["ems_factor"], shaping["ems_offset"])
    for sched, layers in (("flooding", None), ("layered", "greedy")):
        env = dict(NBL_SCHEDULE=sched)
        rc, mean, text = _harness(str(tmp_path), env)
        assert rc == 0 and mean is not None and mean > 1.0 and "Algorithm: Min-Max" in text, text
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rows = hostlib.simulate(str(tmp_path))
        assert len(rows) == 1
        r = rows[0]
        frames = int(r["frames"])
        assert frames >= 64 and frames % P == 0
        L, tx, msg, _ = hostlib.frontend(str(tmp_path), 2.0, frames // P, N, K, code.q, P)
        dec = nb.Decoder(code, nb.METHOD_MINMAX, 10, poll_every=2, layers=layers, minmax=True, **shaping)
        out, conv, its = dec.decode(L)
        dec.close()
        err_sym, err_bit, _ = hostlib.err_count(str(tmp_path), msg, out)
        print("harness", sched, r, "own", int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum()), "iterations per frame", its.mean())
        assert (r["errFrame"], r["errSym"], r["errBit"]) == (int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum())), r
        assert abs(mean - its.mean()) <= 1e-4 * its.mean()
        lay = None if layers is None else nb.layer_greedy(code)
        for b in range(8):                                                # the first frame of every lane against the restatement
            r_out, r_conv, r_its, _, _ = mr.decode(mm, L[b], lay, 10)
            assert (conv[b], its[b]) == (r_conv, r_its) and np.array_equal(out[b], r_out), (sched, b)
    rc, _, text = _harness(str(tmp_path), dict(NBL_SCHEDULE="layered-damped"))
    assert rc != 0 and "DecodeMethod = 3" in text and "NBL_SCHEDULE=flooding or layered" in text, text
    rc, _, text = _harness(str(tmp_path), dict(NBL_SCHEDULE="serial"))
    assert rc != 0 and "NBL_SCHEDULE=serial: unknown schedule" in text, text
    osd = tmp_path / "osd"
    osd.mkdir()
    hostlib.prepare_workdir(str(osd), dict(kw, osd_order=0), GF16, "BPSK")
    rc, _, text = _harness(str(osd), {})
    assert rc != 0 and "DecodeMethod = 3" in text and "OSD" in text, text
