"""Flat fading on a real MI355X (nbl_decode_batch_samples_csi, nbl_decode_batch_samples_idd_csi, nbl_set_fading, nbl_read_gains,
nbl_channel_draws; nbl_demod.hip, nbl_kernels.hip, nbl_fading.hip, nbl_idd.hip) against the numpy restatement of include/nbldpc.h's
definition (tests/fading_ref.py), which tests/test_fading.py holds against a brute force, three anchors and the host layer on the CPU.

  the gain-aware demodulator kernels: the L_ch the decoder saw, max-log / BPSK / q-ary bit for bit, log-sum within fr.LOGSUM_TOL
  the anchors on the device: gain == (1, 0) against the gain-less call, a constant gain against a decoder set up with the pre-faded table
  the Rayleigh channel: gains and samples bit for bit those of the host chain (CComm::Channel_Rayleigh), the draw count, AWGN again
  end to end: the one-call and the two-phase forms, the device transmitter and error count, all against the host chain
  the loop with gains: every output bit for bit against fading_ref's loop on the canonical oracle (tests/test_fading.py asserts the
      convergence mix of the cell); the resident entry point under fading
  the refusals, and the harness switch NBL_CHANNEL / NBL_FADE_BLOCK in every mode the harness has"""
import numpy as np
import pytest

import demod_general as dg
import fading_ref as fr
import idd_ref as ir
import link_shapes as ls
import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
import soft_ref as sr
from nbldpc_amd import hostlib

pytestmark = pytest.mark.gpu

METRICS = {"maxlog": fr.MAXLOG, "logsum": fr.LOGSUM}
SIGMA = fr.KERNEL_SIGMA


def demod_decoder(name, metric, method=nb.METHOD_BP, max_iter=1, points=None, **kw):
    sh = dg.shape(name)
    dec = nb.Decoder(dg.graph(name)[0], method, max_iter, **kw)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"] if points is None else points, metric=metric)
    return dec


def small_decoder(kind, points=None):
    """EMS decoder of fr.small_case(kind) with its BPSK / q-ary demodulator set"""
    N, p, pts, src, rx, gain, sigma, punct = fr.small_case(kind)
    code = nb.Code(dg.U16) if kind == "bpsk" else ls.shape("qary_gf8_punct")[0]
    dec = nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=min(1 << p, 8), ems_nc=2)
    dec.set_demodulator(len(pts), rx.shape[1], src, pts if points is None else points)
    return dec


def lch(dec, B):
    return np.stack([dec.read_lch(b) for b in range(B)])


def same(got, want, tag):
    for what, a, b in zip(("out_sym", "converged", "iters", "passes_used"), got, want):
        assert np.array_equal(a, b), (tag, what, np.flatnonzero(np.asarray(a).reshape(len(a), -1) != np.asarray(b).reshape(len(b), -1))[:8])


# ---- the gain-aware demodulator kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_kernel_equals_the_restatement(name, metric):
    """B = 3, per-sample gains of magnitude 0.03 .. 10 and one exactly (1, 0); without and with a prior"""
    sh, rx, gain, prior = fr.kernel_case(name)
    dec = demod_decoder(name, METRICS[metric])
    for with_prior in (False, True):
        want, scale, _ = fr.kernel_want(name, METRICS[metric], with_prior)
        out, _, _ = dec.decode_samples(rx, SIGMA, prior=prior if with_prior else None, gain=gain)
        got = lch(dec, rx.shape[0])
        err = np.abs(got - want)
        print(f"{name} {metric} prior={with_prior}: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} "
              f"units of 2^-53 (tolerance {fr.LOGSUM_TOL / 2.0 ** -53:.1f})")
        if metric == "maxlog":
            assert sr.bits_equal(got, want), with_prior
        else:
            assert (err <= fr.LOGSUM_TOL * scale).all(), with_prior
        ref, _, _ = dec.decode(got)                                           # and the decode used them
        assert np.array_equal(out, ref)
    dec.decode_samples(rx, SIGMA)                                             # the gains entered: not the gain-less LLRs
    assert not sr.bits_equal(lch(dec, rx.shape[0]), fr.kernel_want(name, METRICS[metric], False)[0])
    dec.close()


@pytest.mark.parametrize("kind", ["bpsk", "qary"])
def test_bpsk_and_qary_kernels_equal_the_restatement(kind):
    N, p, points, src, rx, gain, sigma, punct = fr.small_case(kind)
    want = fr.bpsk_formula(src, rx, gain, sigma, N, p) if kind == "bpsk" else fr.qary_formula(points, src, rx, gain, sigma)
    dec = small_decoder(kind)
    out, _, _ = dec.decode_samples(rx, sigma, gain=gain)
    got = lch(dec, 3)
    assert sr.bits_equal(got, want)
    assert all((got[:, n] == 0).all() for n in punct)
    assert np.array_equal(out, dec.decode(got)[0])
    again = dec.decode_samples(rx, sigma, gain=gain, prior=np.ones((3, N * p)))    # a prior is accepted and inert here
    assert sr.bits_equal(lch(dec, 3), want) and np.array_equal(again[0], out)
    dec.decode_samples(rx, sigma)
    assert not sr.bits_equal(lch(dec, 3), want)
    dec.close()


# ---- the anchors on the device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dg.SHAPES) + ["bpsk", "qary"])
def test_anchor_unit_gain_is_the_gain_less_call(name):
    """gain == (1, 0) through the new instances against gain = None through the old ones: L_ch equal as numbers, every output identical"""
    if name in dg.SHAPES:
        sh, rx, _, prior = fr.kernel_case(name)
        dec = demod_decoder(name, fr.MAXLOG, nb.METHOD_EMS, 3, ems_nm=min(16, sh["q"] // 2), ems_nc=3)
        sigma = SIGMA
    else:
        _, _, _, _, rx, _, sigma, _ = fr.small_case(name)
        dec, prior = small_decoder(name), None
    B = rx.shape[0]
    one = np.zeros_like(rx)
    one[..., 0] = 1.0
    for pr in (None, prior) if prior is not None else (None,):
        base = dec.decode_samples(rx, sigma, prior=pr)
        L0 = lch(dec, B)
        got = dec.decode_samples(rx, sigma, prior=pr, gain=one)
        assert np.array_equal(lch(dec, B), L0)
        for a, b in zip(got, base):
            assert np.array_equal(a, b)
    # gain == NULL IS the existing call
    out = np.zeros((B, dec.code.N), dtype=np.int32)
    rxc = np.ascontiguousarray(rx)
    assert dec.lib.nbl_decode_batch_samples_csi(dec.h, rxc.ctypes.data, None, None, sigma, B, out.ctypes.data, None, None) == 0
    assert np.array_equal(out, dec.decode_samples(rx, sigma)[0])
    dec.close()


CONST_GAIN = (0.6, -1.3)


def prefaded(points):
    pr, pi = fr.faded(np.asarray(points, dtype=np.float64), np.float64(CONST_GAIN[0]), np.float64(CONST_GAIN[1]))
    return np.stack([np.array(pr), np.array(pi)], axis=1)


@pytest.mark.parametrize("name", sorted(dg.SHAPES) + ["qary"])
def test_anchor_constant_gain_is_the_prefaded_table(name):
    """a gain constant over the frame against a decoder whose demodulator was set with the table (pr, pi): bit-identical L_ch and
    identical outputs, on the general max-log path (with and without a prior) and on the q-ary path"""
    if name in dg.SHAPES:
        sh, rx, _, prior = fr.kernel_case(name)
        kw = dict(method=nb.METHOD_EMS, max_iter=3, ems_nm=min(16, sh["q"] // 2), ems_nc=3)
        dec, ref, sigma = demod_decoder(name, fr.MAXLOG, **kw), demod_decoder(name, fr.MAXLOG, points=prefaded(sh["points"]), **kw), SIGMA
    else:
        _, _, points, _, rx, _, sigma, _ = fr.small_case(name)
        dec, ref, prior = small_decoder(name), small_decoder(name, points=prefaded(points)), None
    B = rx.shape[0]
    g = np.ascontiguousarray(np.broadcast_to(np.array(CONST_GAIN), rx.shape))
    for pr in (None, prior) if prior is not None else (None,):
        want = ref.decode_samples(rx, sigma, prior=pr)
        Lw = lch(ref, B)
        got = dec.decode_samples(rx, sigma, prior=pr, gain=g)
        assert sr.bits_equal(lch(dec, B), Lw)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    dec.close()
    ref.close()


# ---- the Rayleigh channel --------------------------------------------------------------------------------------------------------------
def _setup(tmp_path, code_name, cons, method, P, seed, **kw):
    c = df.codes()[code_name]
    q = c["q"]
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=q, code=code_name, method=method, max_iter=10, parallel=P, nqam=(2 if cons == "BPSK" else q),
                                                constellation=cons, random_msg=(1 if cons == "BPSK" else 0), seed=seed, **kw), code_name, cons)
    points = np.array([[x[1], x[2]] for x in sorted(df.constellations()[cons])])
    L = c["N"] * (q.bit_length() - 1) if cons == "BPSK" else c["N"]
    return nb.Code(code_name), points, L, q


CHANNEL_CASES = [(dg.U256, "BPSK", coh) for coh in ("1", "3", "L", "L+5")] + [("BDS.576.288.GF.64", "GRAY_64QAM", "3")]


@pytest.mark.parametrize("code_name,cons,coh", CHANNEL_CASES)
def test_device_channel_bit_identical_to_host_chain(tmp_path, code_name, cons, coh):
    """64 lanes, 2 frames: gains (read_gains) and samples (read_slot_rx) equal CComm::Channel_Rayleigh's bit for bit; channel_draws is
    the advance of the host lanes; decode_noise and the two-phase slot form equal decode_samples(rx, gain=) on the host chain's
    samples and gains; after set_fading(None) the samples are hostlib.channel's again"""
    P, frames, ebn0 = 64, 2, 3.0
    kw = dict(ems_nm=16, ems_nc=3)
    code, points, L, q = _setup(tmp_path, code_name, cons, 2, P, 173, **kw)
    coherence = {"1": 1, "3": 3, "L": L, "L+5": L + 5}[coh]
    rx, gain, txi, state, sigma, draws = hostlib.channel_fading(str(tmp_path), ebn0, frames, L, P, coherence)
    dec = nb.Decoder(code, nb.METHOD_EMS, 4, poll_every=2, **kw)
    dec.set_demodulator(2 if cons == "BPSK" else q, L, np.arange(L), points)
    assert dec.channel_draws() == 4 * L
    dec.set_fading("rayleigh", coherence)
    assert dec.channel_draws() == draws == 4 * L + 4 * (-(-L // coherence))
    for lane in (0, 1, P - 1):
        assert np.array_equal(hostlib.rand_advance(state[lane], dec.channel_draws()), state[P + lane])
    ws = dec.workspace_bytes()
    for f in range(frames):
        sl = slice(f * P, (f + 1) * P)
        slot = f & 1
        dec.channel_batch(slot, txi[sl], state[sl], sigma)
        g, r = dec.read_gains(slot, 0, P), dec.read_slot_rx(slot, 0, P)
        assert sr.bits_equal(g, gain[sl]), f"frame {f}: {int((g.view(np.uint64) != gain[sl].view(np.uint64)).sum())} of {g.size} gain values differ"
        assert sr.bits_equal(r, rx[sl]), f"frame {f}: {int((r.view(np.uint64) != rx[sl].view(np.uint64)).sum())} of {r.size} sample values differ"
        assert sr.bits_equal(dec.read_gains(slot, 3, 2), gain[sl][3:5])
        want = dec.decode_samples(rx[sl], sigma, gain=gain[sl])
        two = dec.decode_resident(slot, sigma, P)
        one = dec.decode_noise(txi[sl], state[sl], sigma)
        for a, b, c in zip(want, two, one):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    assert dec.workspace_bytes() >= ws + 2 * P * L * 16                       # the slots' gains count
    assert not np.array_equal(want[0], dec.decode_samples(rx[sl], sigma)[0])   # (the gains mattered)
    got, frac = dec.channel(txi[:P], state[:P], sigma)
    assert sr.bits_equal(got, rx[:P]) and 0.05 < frac < 0.13, frac
    print(f"{code_name} coherence {coh}: share of log / cos values settled by the host's libm under fading {frac:.4f}")
    # AWGN again
    dec.set_fading(None)
    assert dec.channel_draws() == 4 * L
    rx0, txi0, state0, sigma0 = hostlib.channel(str(tmp_path), ebn0, 1, L, P)
    dec.channel_batch(0, txi0, state0, sigma0)
    assert sr.bits_equal(dec.read_slot_rx(0, 0, P), rx0)
    with pytest.raises(nb.NblError) as e:
        dec.read_gains(0, 0, P)
    assert e.value.status == -1 and "holds no gains" in str(e.value)
    for a, b in zip(dec.decode_resident(0, sigma0, P), dec.decode_samples(rx0, sigma0)):
        assert np.array_equal(a, b)
    # a slot filled before nbl_set_fading decodes as AWGN; the other one still holds its gains
    dec.set_fading("rayleigh", coherence)
    for a, b in zip(dec.decode_resident(0, sigma0, P), dec.decode_samples(rx0, sigma0)):
        assert np.array_equal(a, b)
    if frames > 1:
        assert sr.bits_equal(dec.read_gains(1, 0, P), gain[P:2 * P])
    dec.close()


def test_set_fading_survives_set_demodulator(tmp_path):
    """the setting outlives nbl_set_demodulator and the block count follows the new L"""
    P = 5
    code, points, L, q = _setup(tmp_path, dg.U256, "BPSK", 2, P, 11, ems_nm=16, ems_nc=3)
    dec = nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=16, ems_nc=3)
    pts256 = np.array([[x[1], x[2]] for x in sorted(df.constellations()["GRAY_256QAM"])])
    dec.set_fading("rayleigh", 7)
    assert dec.channel_draws() == 0                                           # (no demodulator yet: L = 0)
    dec.set_demodulator(q, code.N, np.arange(code.N), pts256)
    assert dec.channel_draws() == 4 * code.N + 4 * (-(-code.N // 7))
    rng = np.random.default_rng(3)
    dec.channel_batch(0, rng.integers(0, 256, (P, code.N)).astype(np.uint8), rng.integers(1, 30000, (P, 3)).astype(np.uint32), 0.5)
    dec.set_demodulator(2, L, np.arange(L), points)
    assert dec.channel_draws() == 4 * L + 4 * (-(-L // 7))
    rx, gain, txi, state, sigma, draws = hostlib.channel_fading(str(tmp_path), 2.0, 1, L, P, 7)
    dec.channel_batch(0, txi, state, sigma)
    assert sr.bits_equal(dec.read_slot_rx(0, 0, P), rx) and sr.bits_equal(dec.read_gains(0, 0, P), gain) and draws == dec.channel_draws()
    dec.close()


# ---- end to end with the device transmitter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,coh", [("qary_gf8_punct", 4), ("exchange_msg", 1)])
def test_transmitter_and_error_count_under_fading(tmp_path, name, coh):
    """transmit_batch + decode_resident + count_errors under Rayleigh fading on a link_shapes shape: the slot's gains and samples are the
    host chain's, and the error counts are those of the host chain's ErrCount on decode_samples(rx, gain=)"""
    from link_util import Link
    code, spec, info = ls.shape(name)
    P, frames, ebn0 = 16, 2, 6.0
    link = Link(tmp_path, ls.profile_of(name, P), None, None, P, spec=spec, points=ls.points_of(name))
    _, _, msg, _ = hostlib.frontend(link.dir, ebn0, frames, link.N, link.K, link.q, P)
    rx, gain, txi, state, sigma, draws = hostlib.channel_fading(link.dir, ebn0, frames, link.L, P, coh)
    link.dec.set_fading("rayleigh", coh)
    pns = [pn for pn, _ in link.states(frames, state[:P])]                    # (the PN registers do not depend on the channel)
    for f in range(frames):
        sl, slot = slice(f * P, (f + 1) * P), f & 1
        link.dec.transmit_batch(slot, pns[f], state[sl], sigma)
        m, _, ti = link.dec.read_transmitted(slot, 0, P)
        assert np.array_equal(m, msg[sl]) and np.array_equal(ti, txi[sl])
        assert sr.bits_equal(link.dec.read_gains(slot, 0, P), gain[sl]) and sr.bits_equal(link.dec.read_slot_rx(slot, 0, P), rx[sl])
        got = link.dec.decode_resident(slot, sigma, P)
        want = link.dec.decode_samples(rx[sl], sigma, gain=gain[sl])
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        es, eb, ok = link.dec.count_errors(slot, P)
        hs, hb, hok = hostlib.err_count(link.dir, msg[sl], want[0])
        assert np.array_equal(es, hs) and np.array_equal(eb, hb) and np.array_equal(ok, hok)
    link.dec.close()


# ---- the loop with gains ---------------------------------------------------------------------------------------------------------------
def loop_decoder(poll_every):
    return demod_decoder(fr.LOOP_NAME, fr.MAXLOG, nb.METHOD_EMS, fr.LOOP_MAX_ITER, fixed_iters=0, poll_every=poll_every, **ir.LOOP_EMS)


@pytest.mark.parametrize("poll_every", [0, 2])
def test_loop_with_gains_equals_the_oracle_loop(oracle, poll_every):
    """per-sample gains, max-log on both sides: outputs, flags, iterations and passes_used identical to the restatement's loop.  The
    batch holds codewords that stop at pass 1, at a later pass and never, so the later passes run on gathered survivors whose gains
    must have travelled with them"""
    sh, rx, gain, sigma, _, ref = fr.loop_cell()
    assert ir.has_loop_mix(ref[1], ref[3])
    dec = loop_decoder(poll_every)
    got = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, "maxlog", gain=gain)
    print(f"passes used {np.bincount(got[3], minlength=4)[1:].tolist()}, converged {int(got[1].sum())} of {len(got[1])}")
    same(got, ref, poll_every)
    plain = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, "maxlog")      # without the gains: another result
    assert not np.array_equal(plain[0], got[0])
    one = dec.decode_samples_idd(rx, sigma, 1, "maxlog", gain=gain)          # passes = 1 IS the plain call with gains
    for a, b in zip(one[:3], dec.decode_samples(rx, sigma, gain=gain)):
        assert np.array_equal(a, b)
    # gain == NULL IS the existing call
    out = np.zeros_like(got[0])
    idd = nb.binding.IddParams(ir.LOOP_PASSES, 1)
    rxc = np.ascontiguousarray(rx)
    assert dec.lib.nbl_decode_batch_samples_idd_csi(dec.h, rxc.ctypes.data, None, sigma, rx.shape[0], idd, out.ctypes.data, None, None, None) == 0
    assert np.array_equal(out, plain[0])
    # every codeword alone equals its row
    for b in (0, int(np.flatnonzero(ref[3] > 1)[0]), int(np.flatnonzero(ref[1] == 0)[0])):
        same(dec.decode_samples_idd(rx[b:b + 1], sigma, ir.LOOP_PASSES, "maxlog", gain=gain[b:b + 1]), [x[b:b + 1] for x in ref], b)
    dec.close()


def test_resident_loop_under_fading_equals_the_host_buffer_one(oracle):
    """the samples and gains a slot holds (the device channel's, 96 frames) through nbl_decode_batch_resident_idd against
    nbl_decode_batch_samples_idd_csi on what the slot returns; the GPU's own results hold the convergence mix"""
    sh, _, _, sigma, _, _ = fr.loop_cell()
    B = 96
    dec = loop_decoder(2)
    dec.set_fading("rayleigh", 1)
    state = np.random.default_rng(9).integers(1, 30000, (B, 3)).astype(np.uint32)
    dec.channel_batch(0, np.zeros((B, sh["L"]), dtype=np.uint8), state, sigma)
    rx, gain = dec.read_slot_rx(0, 0, B), dec.read_gains(0, 0, B)
    host = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, "maxlog", gain=gain)
    res = dec.decode_resident(0, sigma, B, passes=ir.LOOP_PASSES, soft="maxlog")
    same(res, host, "resident")
    print(f"passes used {np.bincount(host[3], minlength=4)[1:].tolist()}, converged {int(host[1].sum())} of {B}")
    assert ir.has_loop_mix(host[1], host[3]), (host[1].tolist(), host[3].tolist())
    assert sr.bits_equal(dec.read_slot_rx(0, 0, B), rx) and sr.bits_equal(dec.read_gains(0, 0, B), gain)   # only ever read
    dec.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    P = 4
    code, points, L, q = _setup(tmp_path, dg.U256, "BPSK", 2, P, 5, ems_nm=16, ems_nc=3)
    dec = nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=16, ems_nc=3)
    dec.set_demodulator(2, L, np.arange(L), points)
    dec.set_fading("rayleigh", 3)
    draws = dec.channel_draws()
    for model, coherence, text in ((2, 3, "unknown model 2"), (-1, 1, "unknown model -1"), (1, 0, "coherence must be at least 1, got 0"),
                                   (1, -4, "coherence must be at least 1, got -4")):
        with pytest.raises(nb.NblError) as e:
            dec.set_fading(model, coherence)
        assert e.value.status == -1 and "nbl_set_fading" in str(e.value) and text in str(e.value)
        assert dec.channel_draws() == draws                                   # the previous setting is still in force
    assert dec.lib.nbl_set_fading(None, None) == -1
    with pytest.raises(nb.NblError) as e:                                     # a slot that holds nothing
        dec.read_gains(0, 0, 1)
    assert e.value.status == -1 and "holds no gains" in str(e.value)
    rx, gain, txi, state, sigma, _ = hostlib.channel_fading(str(tmp_path), 2.0, 1, L, P, 3)
    dec.channel_batch(1, txi, state, sigma)
    assert sr.bits_equal(dec.read_gains(1, 0, P), gain)
    with pytest.raises(nb.NblError) as e:
        dec.read_gains(1, 2, P)
    assert e.value.status == -1 and "does not hold these lanes" in str(e.value)
    dec.set_fading(None)
    dec.channel_batch(1, txi, state, sigma)                                   # an AWGN batch: the slot's gains are gone
    with pytest.raises(nb.NblError) as e:
        dec.read_gains(1, 0, P)
    assert e.value.status == -1 and "holds no gains" in str(e.value)
    # the calls they extend refuse the same things
    out = np.zeros((P, code.N), dtype=np.int32)
    fresh = nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=16, ems_nc=3)
    rxc, gc = np.ascontiguousarray(rx), np.ascontiguousarray(gain)
    assert fresh.lib.nbl_decode_batch_samples_csi(fresh.h, rxc.ctypes.data, gc.ctypes.data, None, sigma, P, out.ctypes.data, None, None) == -1
    assert "nbl_set_demodulator has not been called" in fresh.lib.nbl_last_error(fresh.h).decode()
    idd = nb.binding.IddParams(0, 1)
    fresh.set_demodulator(2, L, np.arange(L), points)
    assert fresh.lib.nbl_decode_batch_samples_idd_csi(fresh.h, rxc.ctypes.data, gc.ctypes.data, sigma, P, idd, out.ctypes.data, None, None, None) == -1
    text = fresh.lib.nbl_last_error(fresh.h).decode()
    assert "nbl_decode_batch_samples_idd_csi" in text and "passes must be at least 1, got 0" in text
    assert fresh.lib.nbl_decode_batch_samples_csi(fresh.h, rxc.ctypes.data, gc.ctypes.data, None, -1.0, P, out.ctypes.data, None, None) == -1
    fresh.close()
    dec.close()


# ---- the harness switch ------------------------------------------------------------------------------------------------------------------
HARNESS_KW = dict(gfq=16, method=2, max_iter=4, ems_nm=8, ems_nc=2, parallel=8, crc_len=8, random_msg=1, min_sim_cycle=16, snr_begin=6.0, snr_step=1.0,
                  snr_stop=6.0)
MODES = {"host channel, device demodulator": {"NBL_DEVICE_NOISE": "0"}, "device channel": {}, "device channel, serial": {"NBL_PIPELINE": "0"},
         "device transmitter": {"NBL_DEVICE_TX": "1"}, "device transmitter, serial": {"NBL_DEVICE_TX": "1", "NBL_PIPELINE": "0"},
         "host demodulator": {"NBL_DEVICE_DEMOD": "0"}}
SWITCHES = ("NBL_DEVICE_NOISE", "NBL_PIPELINE", "NBL_DEVICE_TX", "NBL_DEVICE_DEMOD")


@pytest.mark.parametrize("cons", ["BPSK", "GRAY_64QAM"])
def test_harness_channel_switch(tmp_path, monkeypatch, cons):
    """NBL_CHANNEL=rayleigh at one Eb/N0 on divsalar.UNBLDPC.128.64.GF.16: for NBL_FADE_BLOCK 1 and L the row is the same whether the
    channel runs on the host behind the device demodulator, on the device, behind the device transmitter, pipelined or serial, or
    with the demodulator on the host (BPSK: bit-identical LLRs; 64-QAM over GF(16) takes the general demodulator, max-log); with
    NBL_IDD_PASSES=2 on the general demodulator the host-channel and device-channel rows agree too.  On BPSK at 6 dB the rows are
    not the AWGN row, and the two block lengths give different rows."""
    for k in SWITCHES + ("NBL_CHANNEL", "NBL_FADE_BLOCK", "NBL_IDD_PASSES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("NBL_DEMOD_METRIC", "maxlog")
    kw = dict(HARNESS_KW, nqam=2 if cons == "BPSK" else 64)
    if cons != "BPSK":                                                        # (64-QAM under Rayleigh fading wants more: at 6 dB every frame fails)
        kw.update(snr_begin=12.0, snr_stop=12.0)
    hostlib.prepare_workdir(str(tmp_path), kw, dg.U16, cons)
    N = df.codes()[dg.U16]["N"]
    L = N * 4 if cons == "BPSK" else N * 4 // 6
    awgn = hostlib.simulate(str(tmp_path))
    monkeypatch.setenv("NBL_CHANNEL", "awgn")
    assert hostlib.simulate(str(tmp_path)) == awgn                            # the default
    monkeypatch.setenv("NBL_CHANNEL", "rayleigh")
    rows = {}
    for block in (1, L):
        monkeypatch.setenv("NBL_FADE_BLOCK", str(block))
        for mode, env in MODES.items():
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            rows[block, mode] = hostlib.simulate(str(tmp_path))
            assert len(rows[block, mode]) == 1
            print(block, mode, rows[block, mode][0])
        for mode in MODES:
            assert rows[block, mode] == rows[block, "device channel"], (block, mode)
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        if cons != "BPSK":                                                    # the loop, host channel against device channel
            monkeypatch.setenv("NBL_IDD_PASSES", "2")
            two = hostlib.simulate(str(tmp_path))
            monkeypatch.setenv("NBL_DEVICE_NOISE", "0")
            assert hostlib.simulate(str(tmp_path)) == two
            monkeypatch.delenv("NBL_DEVICE_NOISE")
            monkeypatch.delenv("NBL_IDD_PASSES")
        if cons == "BPSK":                                                    # (at 6 dB: no frame error over AWGN, several under fading)
            assert rows[block, "device channel"] != awgn
    monkeypatch.delenv("NBL_FADE_BLOCK")
    assert hostlib.simulate(str(tmp_path)) == rows[1, "device channel"]       # NBL_FADE_BLOCK defaults to 1
    if cons == "BPSK":
        assert rows[1, "device channel"] != rows[L, "device channel"]


def test_harness_switch_refusals(tmp_path, monkeypatch, capfd):
    def refused(text):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            hostlib.simulate(str(tmp_path))
        err = capfd.readouterr().err
        assert text in err, (text, err)
    hostlib.prepare_workdir(str(tmp_path), dict(HARNESS_KW, nqam=2), dg.U16, "BPSK")
    monkeypatch.setenv("NBL_CHANNEL", "rician")
    refused("NBL_CHANNEL=rician: unknown channel (awgn, rayleigh)")
    monkeypatch.setenv("NBL_CHANNEL", "rayleigh")
    for bad in ("0", "-3", "x", "2x", ""):
        monkeypatch.setenv("NBL_FADE_BLOCK", bad)
        refused(f"NBL_FADE_BLOCK={bad}: the number of samples that share one gain must be an integer from 1 up")
