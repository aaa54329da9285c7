"""The general demodulator kernel (nbldpc_amd/csrc/nbl_demod.hip; modulation orders other than 2 and q) against the numpy float64
restatement of include/nbldpc.h's definition (tests/demod_general.py): the L_ch the decoder saw, read back after a decode call.
Max-log bit for bit; log-sum within dg.LOGSUM_TOL (four times the restatement's own measured error); the same
kernel forced onto M = 2 and M = q against the two reference-pinned kernels within dg.ANCHOR_EPS (derived there); the device link
chain against the host chain under max-log; the refusals.  The reference computes none of these LLRs: no value here is its."""
import functools

import numpy as np
import pytest

import demod_general as dg
import nbldpc_amd as nb
from nbldpc_amd import hostlib

pytestmark = pytest.mark.gpu

B, SIGMA, SEED = 3, 0.4, 11
METRICS = {"maxlog": dg.MAXLOG, "logsum": dg.LOGSUM}


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def case(name, metric):
    """(shape, rx, restatement, scale), computed once per (shape, metric) and shared"""
    sh = dg.shape(name)
    rx, _ = dg.samples(sh, B, SIGMA, SEED)
    want, scale = dg.demod(sh["points"], sh["src"], rx, SIGMA, sh["N"], sh["p"], metric)
    for x in (rx, want, scale):
        x.setflags(write=False)
    return sh, rx, want, scale


def decoder(name, metric, **kw):
    sh = dg.shape(name)
    dec = nb.Decoder(dg.graph(name)[0], nb.METHOD_BP, 1, **kw)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=metric)
    return dec


def seen_lch(dec, rx, sigma):
    """the channel LLRs the decoder worked from, [B][N][q-1]"""
    out, _, _ = dec.decode_samples(rx, sigma)
    return np.stack([dec.read_lch(b) for b in range(rx.shape[0])]), out


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_kernel_equals_the_restatement(name, metric):
    sh, rx, want, scale = case(name, METRICS[metric])
    dec = decoder(name, METRICS[metric])
    got, out = seen_lch(dec, rx, SIGMA)
    err = np.abs(got - want)
    print(f"{name} {metric}: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} units of 2^-53")
    if metric == "maxlog":
        assert bits_equal(got, want)
    else:
        assert (err <= dg.LOGSUM_TOL * scale).all()
    # and the decode used them: the same words as from the same LLRs handed over as L_ch
    ref, _, _ = dec.decode(got)
    assert np.array_equal(out, ref)
    dec.close()


def test_force_general_bpsk_equals_the_bpsk_kernel():
    code = nb.Code(dg.U16)
    N, p, punct = code.N, 4, (5,)
    L = (N - 1) * p
    src = dg.src_table(N, p, punct, 1, L)
    points = dg.named_points("BPSK")
    rng = np.random.default_rng(SEED)
    rx = points[rng.integers(0, 2, (B, L))] + SIGMA * rng.standard_normal((B, L, 2))
    dec = nb.Decoder(code, nb.METHOD_BP, 1)
    dec.set_demodulator(2, L, src, points)
    old, _ = seen_lch(dec, rx, SIGMA)
    assert bits_equal(old, dg.bpsk_formula(src, rx[:, :, 0], SIGMA, N, p))
    _, scale = dg.demod(points, src, rx, SIGMA, N, p, dg.MAXLOG)
    for metric in (dg.MAXLOG, dg.LOGSUM):
        dec.set_demodulator(2, L, src, points, metric=metric, force_general=True)
        new, _ = seen_lch(dec, rx, SIGMA)
        assert bits_equal(new, dg.demod(points, src, rx, SIGMA, N, p, metric)[0])    # no foreign bit: both metrics exact
        err = np.abs(new - old)
        print(f"BPSK: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} units of 2^-53 (bound 16)")
        assert (err <= dg.ANCHOR_EPS * scale).all() and not new[:, 5].any()
    dec.close()


def test_force_general_qary_equals_the_qary_kernel():
    code, _ = dg.graph("gf64_16qam")
    N, p, punct = code.N, 6, (3,)
    src, L = dg.qary_src(N, p, punct)
    src_sym = np.array([-1 if n in punct else n - sum(x < n for x in punct) for n in range(N)], dtype=np.int32)
    points = dg.named_points("GRAY_64QAM")
    rng = np.random.default_rng(SEED)
    rx = points[rng.integers(0, 64, (B, L))] + SIGMA * rng.standard_normal((B, L, 2))
    dec = nb.Decoder(code, nb.METHOD_BP, 1)
    dec.set_demodulator(64, L, src_sym, points)
    old, _ = seen_lch(dec, rx, SIGMA)
    assert bits_equal(old, dg.qary_formula(points, src_sym, rx, SIGMA))
    want, scale = dg.demod(points, src, rx, SIGMA, N, p, dg.MAXLOG)
    dec.set_demodulator(64, L, src, points, metric=dg.LOGSUM, force_general=True)
    new, _ = seen_lch(dec, rx, SIGMA)
    err = np.abs(new - old)
    print(f"q-ary: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} units of 2^-53 (bound 16)")
    assert bits_equal(new, want) and (err <= dg.ANCHOR_EPS * scale).all() and not new[:, 3].any()
    dec.close()


def test_batch_above_max_batch():
    name = "gf64_16qam"
    sh = dg.shape(name)
    rx, _ = dg.samples(sh, 7, SIGMA, SEED + 1)
    want, _ = dg.demod(sh["points"], sh["src"], rx, SIGMA, sh["N"], sh["p"], dg.MAXLOG)
    dec = decoder(name, dg.MAXLOG, max_batch=2)
    got, _ = seen_lch(dec, rx[:2], SIGMA)
    assert bits_equal(got, want[:2])
    got, _ = seen_lch(dec, rx, SIGMA)
    assert bits_equal(got, want)
    dec.close()


CHAIN = {"gf16_qpsk": (dg.U16, "GRAY_QPSK", 16), "gf256_64qam": (dg.U256, "GRAY_64QAM", 256)}


@pytest.mark.parametrize("name", sorted(CHAIN))
def test_device_chain_equals_the_host_chain(tmp_path, monkeypatch, name):
    """transmitter, channel, general demodulator, decode and error count on the device against the host chain of the same profile,
    under max-log (the one metric under which host and device LLRs are bit-identical)"""
    monkeypatch.setenv("NBL_DEMOD_METRIC", "maxlog")
    code_name, cons, q = CHAIN[name]
    P, p = 4, q.bit_length() - 1
    points = dg.named_points(cons)
    M = len(points)
    m = M.bit_length() - 1
    ems = dict(ems_nm=min(32, q // 2), ems_nc=2)                                # nm may not exceed q
    kw = dict(gfq=q, method=2, max_iter=4, parallel=P, nqam=M, crc_len=8, random_msg=1, **ems)
    hostlib.prepare_workdir(str(tmp_path), kw, code_name, cons)
    code = nb.Code(code_name)
    N, K = code.N, code.N - code.M
    L = N * p // m
    src = dg.src_table(N, p, (), m, L)
    Lh, tx, msg, sigma = hostlib.frontend(str(tmp_path), 5.0, 1, N, K, q, P)
    rx, txi, state, sigma2 = hostlib.channel(str(tmp_path), 5.0, 1, L, P)
    assert sigma == sigma2
    assert np.array_equal(txi, dg.puncture_modulate(tx, p, (), m, L))          # the host's Modulate is the restatement's
    assert bits_equal(Lh, dg.demod(points, src, rx, sigma, N, p, dg.MAXLOG)[0])
    dec = nb.Decoder(code, 2, 4, poll_every=2, **ems)
    dec.set_demodulator(M, L, src, points, metric=dg.MAXLOG)
    dec.set_transmitter(gen=hostlib.generator(str(tmp_path), N, K), crc_len=8, random_msg=1, parallel=P, punct=[], mod_order=M, n_mod_sym=L)
    pn = np.array([hostlib.pn_initial(i) for i in range(P)], dtype=np.uint16)
    dec.transmit_batch(0, pn, state, sigma)
    dmsg, dcode, dtxi = dec.read_transmitted(0, 0, P)
    assert np.array_equal(dcode, tx) and np.array_equal(dmsg, msg)
    assert np.array_equal(dtxi, dg.puncture_modulate(tx, p, (), m, L))         # tx_index against the Python Modulate
    assert bits_equal(dec.read_slot_rx(0, 0, P), rx)                           # samples
    out, conv, iters = dec.decode_resident(0, sigma, P)
    assert bits_equal(np.stack([dec.read_lch(b) for b in range(P)]), Lh)       # LLRs: host chain == device chain
    for a, b in zip((out, conv, iters), dec.decode(Lh)):                       # decoded words
        assert np.array_equal(a, b)
    for a, b in zip(dec.count_errors(0, P), hostlib.err_count(str(tmp_path), msg, out)):   # error counts
        assert np.array_equal(a, b)
    # the other consumers of the demodulator: host samples, and host indices with the channel on the device
    for a, b in zip(dec.decode_samples(rx, sigma), (out, conv, iters)):
        assert np.array_equal(a, b)
    for a, b in zip(dec.decode_noise(txi, state, sigma), (out, conv, iters)):
        assert np.array_equal(a, b)
    dec.close()


def test_simulation_counts_do_not_depend_on_where_the_transmitter_runs(tmp_path, monkeypatch):
    """the harness on GF(16) N = 32 (128 bits) over Gray QPSK under max-log, 320 frames at a point with frame errors"""
    monkeypatch.setenv("NBL_DEMOD_METRIC", "maxlog")
    kw = dict(gfq=16, method=2, max_iter=5, ems_nm=8, ems_nc=2, parallel=8, nqam=4, crc_len=8, random_msg=1, min_sim_cycle=320,
              snr_begin=2.0, snr_step=1.0, snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, dg.U16, "GRAY_QPSK")
    rows = {}
    for tx in ("0", "1"):
        monkeypatch.setenv("NBL_DEVICE_TX", tx)
        rows[tx] = hostlib.simulate(str(tmp_path))
    assert len(rows["0"]) == 1 and rows["0"] == rows["1"], rows
    r = rows["0"][0]
    assert r["frames"] >= 320 and 0 < r["errFrame"] < r["frames"] and r["errSym"] > 0 and r["errBit"] > 0, r


def test_refusals_leave_the_demodulator_usable():
    name = "gf64_16qam"
    sh, rx, want, _ = case(name, dg.MAXLOG)
    dec = decoder(name, dg.MAXLOG)
    twice = sh["src"].copy()
    twice[7] = twice[2]
    beyond = sh["src"].copy()
    beyond[4] = sh["L"] * sh["m"]
    bad = [dict(src=twice), dict(src=beyond), dict(mod_order=3), dict(mod_order=512), dict(metric=2), dict(constellation=None),
           dict(mod_order=0), dict(mod_order=2, metric=7), dict(mod_order=64, force_general=True, constellation=None)]
    for over in bad:
        a = dict(mod_order=sh["M"], n_mod_sym=sh["L"], src=sh["src"], constellation=sh["points"], metric=dg.MAXLOG)
        a.update(over)
        with pytest.raises(nb.NblError) as e:
            dec.set_demodulator(**a)
        assert e.value.status == -1 and str(e.value).split(":", 1)[1].strip(), (over, e.value)
        got, _ = seen_lch(dec, rx, SIGMA)
        assert bits_equal(got, want), over
    dec.close()
