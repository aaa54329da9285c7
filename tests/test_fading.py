"""Flat fading on the CPU: the numpy restatement of include/nbldpc.h's demodulators with gains (tests/fading_ref.py) against a
probability-domain brute force and the three anchors that tie it to the gain-less, reference-pinned paths; the host layer (the gain
overload of CComm::DemodulateGeneral, the BPSK and q-ary expressions with gains, CComm::Channel_Rayleigh) against the restatement; and
the convergence mix the loop cell of tests/test_gpu_fading.py must hold, per the canonical oracle.  No GPU; the reference computes none
of this, so no value here is its."""
import numpy as np
import pytest

import demod_general as dg
import fading_ref as fr
import idd_ref as ir
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib

METRICS = {"maxlog": fr.MAXLOG, "logsum": fr.LOGSUM}
SIGMA = fr.KERNEL_SIGMA


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def within(got, want, scale, eps, what):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble))
    ratio = float((err / np.where(scale > 0, scale, 1.0)).max())
    print(f"{what}: worst error / scale = {ratio / 2.0 ** -53:.3f} units of 2^-53 (bound {eps / 2.0 ** -53:.1f})")
    return bool((err <= eps * scale).all())


# ---- host layer against restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_host_layer_equals_the_restatement(name, with_prior):
    """CComm::DemodulateGeneral with gains, B = 3, random per-sample gains of magnitude 0.03 .. 10 and one exactly (1, 0): max-log bit
    for bit; log-sum within four times the float64 restatement's own error against the longdouble one on these faded inputs (floor
    dg.ANCHOR_EPS); gain = NULL IS the gain-less function"""
    sh, rx, gain, prior = fr.kernel_case(name)
    pr = prior if with_prior else None
    args = (sh["N"], sh["p"], sh["points"], sh["src"], rx)
    want, scale, _ = fr.kernel_want(name, fr.MAXLOG, with_prior)
    got = hostlib.demod_csi("general", *args, gain, SIGMA, fr.MAXLOG, pr)
    assert bits_equal(got, want) and np.isfinite(got).all()
    want_ls, scale, own = fr.kernel_want(name, fr.LOGSUM, with_prior)
    print(f"{name}: float64 restatement against longdouble, worst error / scale = {own / 2.0 ** -53:.2f} units of 2^-53 "
          f"(recorded {fr.FADED_LOGSUM_ERR / 2.0 ** -53:.1f})")
    assert own <= 1.25 * fr.FADED_LOGSUM_ERR                                  # (the record is not stale; the slack is demod_general's)
    ls = hostlib.demod_csi("general", *args, gain, SIGMA, fr.LOGSUM, pr)
    assert within(ls, want_ls, scale, fr.LOGSUM_TOL, f"{name} host log-sum")
    for metric in (fr.MAXLOG, fr.LOGSUM):
        assert bits_equal(hostlib.demod_csi("general", *args, None, SIGMA, metric, pr), hostlib.demod_general_prior(*args, SIGMA, metric, pr))
    assert not bits_equal(got, hostlib.demod_general_prior(*args, SIGMA, fr.MAXLOG, pr))   # (the gains entered)
    if with_prior and name != "gf16_qpsk_aligned":                            # (and so did the prior)
        assert not bits_equal(got, fr.kernel_want(name, fr.MAXLOG, False)[0])


@pytest.mark.parametrize("name", ir.DISCRIMINATING)
def test_restatement_equals_the_brute_force(name):
    """log-sum in numpy.longdouble against sum over c of P(c) exp(-|y - h c|^2 / 2 sigma^2) in complex arithmetic; two label bits
    unclaimed; gains and prior must matter on these inputs, so a sign, conjugation or bit-order error is O(1)"""
    sh, src, rx, gain, prior = fr.brute_case(name)
    assert np.finfo(np.longdouble).nmant >= 63
    assert (ir.claims(src, sh["L"], sh["m"]) < 0).sum() >= 2
    got, _ = fr.demod(sh["points"], src, rx, gain, 0.4, sh["N"], sh["p"], fr.LOGSUM, prior, np.longdouble)
    want = fr.brute_force(sh["points"], src, rx, gain, 0.4, sh["N"], sh["p"], prior)
    no_prior, _ = fr.demod(sh["points"], src, rx, gain, 0.4, sh["N"], sh["p"], fr.LOGSUM, None, np.longdouble)
    conj = gain * np.array([1.0, -1.0])
    no_gain, _ = fr.demod(sh["points"], src, rx, conj, 0.4, sh["N"], sh["p"], fr.LOGSUM, prior, np.longdouble)
    err = float((np.abs(got - want) / np.maximum(1, np.abs(want))).max())
    print(f"{name}: worst |restatement - brute force| / max(1, |L|) = {err:.3e} (recorded {fr.BRUTE_FORCE_ERR:.3e}, bound {fr.BRUTE_FORCE_TOL:.3e}); "
          f"largest |L| {float(np.abs(want).max()):.1f}, the prior moves the LLRs by up to {float(np.abs(got - no_prior).max()):.1f}, "
          f"the conjugate gain by up to {float(np.abs(got - no_gain).max()):.1f}")
    assert float(np.abs(got - no_prior).max()) > 1.0 and float(np.abs(got - no_gain).max()) > 1.0
    assert err <= fr.BRUTE_FORCE_TOL


# ---- BPSK and q-ary expressions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bpsk", "qary"])
def test_bpsk_and_qary_expressions_with_gains(kind):
    """host layer against restatement, bit for bit, on divsalar.UNBLDPC.128.64.GF.16 (BPSK) and qary_gf8_punct (punctured symbols
    stay 0.0); the gains enter"""
    N, p, points, src, rx, gain, sigma, punct = fr.small_case(kind)
    got = hostlib.demod_csi(kind, N, p, points, src, rx, gain, sigma)
    if kind == "bpsk":
        want = fr.bpsk_formula(src, rx, gain, sigma, N, p)
        plain = dg.bpsk_formula(src, rx[..., 0], sigma, N, p)
    else:
        want = fr.qary_formula(points, src, rx, gain, sigma)
        plain = dg.qary_formula(points, src, rx, sigma)
        assert len(punct) >= 3 and all((got[:, n] == 0).all() for n in punct)
    assert bits_equal(got, want) and np.isfinite(got).all()
    assert not bits_equal(got, plain)


# ---- the three anchors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_anchor_unit_gain(name):
    """gain == (1, 0) everywhere: the gain-less result, compared as numbers (the sign of a zero may differ) -- restatement and host
    layer, both metrics, with and without a prior"""
    sh, rx, _, prior = fr.kernel_case(name)
    one = np.zeros_like(rx)
    one[..., 0] = 1.0
    args = (sh["points"], sh["src"], rx)
    for metric in (fr.MAXLOG, fr.LOGSUM):
        for pr in (None, prior):
            plain = dg.demod(*args, SIGMA, sh["N"], sh["p"], metric)[0] if pr is None else ir.demod_prior(*args, SIGMA, sh["N"], sh["p"], metric, pr)[0]
            got, _ = fr.demod(*args, one, SIGMA, sh["N"], sh["p"], metric, pr)
            assert np.array_equal(got, plain), (name, metric)
            host = hostlib.demod_csi("general", sh["N"], sh["p"], sh["points"], sh["src"], rx, one, SIGMA, metric, pr)
            assert np.array_equal(host, hostlib.demod_general_prior(sh["N"], sh["p"], sh["points"], sh["src"], rx, SIGMA, metric, pr)), (name, metric)


def test_anchor_unit_gain_bpsk_and_qary():
    for kind in ("bpsk", "qary"):
        N, p, points, src, rx, gain, sigma, _ = fr.small_case(kind)
        one = np.zeros_like(rx)
        one[..., 0] = 1.0
        plain = dg.bpsk_formula(src, rx[..., 0], sigma, N, p) if kind == "bpsk" else dg.qary_formula(points, src, rx, sigma)
        want = fr.bpsk_formula(src, rx, one, sigma, N, p) if kind == "bpsk" else fr.qary_formula(points, src, rx, one, sigma)
        assert np.array_equal(want, plain)
        assert np.array_equal(hostlib.demod_csi(kind, N, p, points, src, rx, one, sigma), plain)


CONST_GAIN = (0.6, -1.3)


def prefaded(points, g=CONST_GAIN):
    pr, pi = fr.faded(np.asarray(points, dtype=np.float64), np.float64(g[0]), np.float64(g[1]))
    return np.stack([np.array(pr), np.array(pi)], axis=1)


@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_anchor_constant_gain_is_the_prefaded_table(name):
    """a gain constant over the frame: bit-identical to the gain-less restatement on the table (pr, pi) -- max-log, and the host layer"""
    sh, rx, _, prior = fr.kernel_case(name)
    g = np.broadcast_to(np.array(CONST_GAIN), rx.shape)
    table = prefaded(sh["points"])
    for pr in (None, prior):
        plain = dg.demod(table, sh["src"], rx, SIGMA, sh["N"], sh["p"], dg.MAXLOG)[0] if pr is None else ir.demod_prior(table, sh["src"], rx, SIGMA, sh["N"], sh["p"], ir.MAXLOG, pr)[0]
        got, _ = fr.demod(sh["points"], sh["src"], rx, g, SIGMA, sh["N"], sh["p"], fr.MAXLOG, pr)
        assert bits_equal(got, plain), name
        assert bits_equal(hostlib.demod_csi("general", sh["N"], sh["p"], sh["points"], sh["src"], rx, g, SIGMA, fr.MAXLOG, pr), plain), name


def test_anchor_constant_gain_qary():
    N, p, points, src, rx, _, sigma, _ = fr.small_case("qary")
    g = np.broadcast_to(np.array(CONST_GAIN), rx.shape)
    plain = dg.qary_formula(prefaded(points), src, rx, sigma)
    assert bits_equal(fr.qary_formula(points, src, rx, g, sigma), plain)
    assert bits_equal(hostlib.demod_csi("qary", N, p, points, src, rx, g, sigma), plain)


def test_anchor_real_gain_bpsk():
    """a real positive gain g per sample: the gain-less BPSK LLRs of the samples g * re"""
    N, p, points, src, rx, gain, sigma, _ = fr.small_case("bpsk")
    g = np.zeros_like(gain)
    g[..., 0] = np.hypot(gain[..., 0], gain[..., 1])
    plain = dg.bpsk_formula(src, g[..., 0] * rx[..., 0], sigma, N, p)
    assert bits_equal(fr.bpsk_formula(src, rx, g, sigma, N, p), plain)
    assert bits_equal(hostlib.demod_csi("bpsk", N, p, points, src, rx, g, sigma), plain)


# ---- the host layer's Rayleigh channel -----------------------------------------------------------------------------------------------
U256 = dg.U256
RAY_P, RAY_FRAMES, RAY_EBN0 = 8, 2, 3.0


@pytest.fixture(scope="module")
def ray_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("rayleigh")
    hostlib.prepare_workdir(str(d), dict(gfq=256, code=U256, method=2, max_iter=4, parallel=RAY_P, nqam=2, constellation="BPSK", random_msg=1, seed=321,
                                         ems_nm=16, ems_nc=3), U256, "BPSK")
    return str(d)


@pytest.mark.parametrize("coh", ["1", "3", "L", "L+5"])
def test_host_channel_rayleigh(ray_dir, coh):
    """CComm::Channel_Rayleigh on divsalar.UNBLDPC.128.64.GF.256 BPSK (L = 128), 8 lanes, 2 frames: gains constant inside blocks and
    changing between them; samples and gains bit for bit those of the header's frame restated on CRand in Python (the noise is the AWGN
    noise of the state moved on 4 nblk draws); the lane state after each frame; the mean of |h|^2"""
    L = df.codes()[U256]["N"] * 8
    coherence = {"1": 1, "3": 3, "L": L, "L+5": L + 5}[coh]
    nblk = -(-L // coherence)
    rx, gain, txi, state, sigma, draws = hostlib.channel_fading(ray_dir, RAY_EBN0, RAY_FRAMES, L, RAY_P, coherence)
    _, txi0, state0, sigma0 = hostlib.channel(ray_dir, RAY_EBN0, RAY_FRAMES, L, RAY_P)
    assert draws == 4 * nblk + 4 * L and sigma == sigma0 and np.array_equal(txi, txi0) and np.array_equal(state[:RAY_P], state0[:RAY_P])
    points = dg.named_points("BPSK")
    # blocks
    for k in range(nblk):
        blk = gain[:, k * coherence:(k + 1) * coherence]
        assert bits_equal(blk, np.broadcast_to(blk[:, :1], blk.shape)), k
    first = gain[:, ::coherence]
    if nblk > 1:
        assert (first[:, 1:] != first[:, :-1]).any(axis=2).all()
    # the frame restated, three lanes of the first frame and one of the second
    for b in (0, 1, RAY_P - 1, RAY_P + 2):
        want_rx, want_gain, after = fr.rayleigh_frame(state[b], points[txi[b]], sigma, coherence)
        assert bits_equal(gain[b], want_gain) and bits_equal(rx[b], want_rx), b
        assert np.array_equal(after, hostlib.rand_advance(state[b], draws)), b
        noise = fr.awgn_noise(hostlib.rand_advance(state[b], 4 * nblk), L, sigma)
        c = points[txi[b]]
        pr = gain[b, :, 0] * c[:, 0] - gain[b, :, 1] * c[:, 1]
        pi = gain[b, :, 0] * c[:, 1] + gain[b, :, 1] * c[:, 0]
        assert bits_equal(rx[b], np.stack([pr + noise[:, 0], pi + noise[:, 1]], axis=1)), b
    # the lane state after each frame
    for lane in range(RAY_P):
        assert np.array_equal(hostlib.rand_advance(state[lane], draws), state[RAY_P + lane]), lane
    # E|h|^2 = 1: |h|^2 is exponential with unit variance, so the mean over n independent gains has standard deviation 1 / sqrt(n)
    h2 = (first ** 2).sum(axis=2).ravel()
    print(f"coherence {coh}: {h2.size} gains, mean |h|^2 = {h2.mean():.4f}")
    assert abs(h2.mean() - 1.0) <= 5.0 / np.sqrt(h2.size)


# ---- the loop cell -------------------------------------------------------------------------------------------------------------------
def test_loop_cell_holds_the_convergence_mix(oracle):
    """a condition of tests/test_gpu_fading.py, not a measurement: per the oracle's loop with gains the cell has frames that converge
    in pass 1, one or more in a later pass, two or more never; and the gains matter: the loop without them decodes other words"""
    sh, rx, gain, sigma, max_iter, (out, conv, its, used) = fr.loop_cell()
    never = int((conv == 0).sum())
    by_pass = [int(((conv == 1) & (used == k)).sum()) for k in range(1, ir.LOOP_PASSES + 1)]
    print(f"converged in pass 1 / 2 / 3: {by_pass}, never: {never}")
    assert ir.has_loop_mix(conv, used), (by_pass, never)
    assert (used[conv == 0] == ir.LOOP_PASSES).all() and ((used >= 1) & (used <= ir.LOOP_PASSES)).all()
