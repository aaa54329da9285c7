"""Iterative demapping on the CPU: the numpy restatement of include/nbldpc.h's prior-aware demodulator (tests/idd_ref.py) against the
prior-less restatement, a probability-domain brute force and two factorising anchors; the host layer (the prior-aware overload of
CComm::DemodulateGeneral) against the restatement; and the convergence mix the loop cells of tests/test_gpu_idd.py must hold, per
the canonical oracle.  No GPU; the reference computes none of this, so no value here is its."""
import numpy as np
import pytest

import demod_general as dg
import idd_ref as ir
from nbldpc_amd import hostlib

METRICS = {"maxlog": ir.MAXLOG, "logsum": ir.LOGSUM}


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_zero_prior_is_the_prior_less_demodulator(name, metric):
    """d' = d - (2 sigma^2) * 0.0 = d exactly: bit for bit, also with a prior of -0.0"""
    sh, rx, prior = ir.kernel_case(name)
    want, _ = dg.demod(sh["points"], sh["src"], rx, ir.KERNEL_SIGMA, sh["N"], sh["p"], METRICS[metric])
    for zero in (0.0, -0.0):
        got, _ = ir.demod_prior(sh["points"], sh["src"], rx, ir.KERNEL_SIGMA, sh["N"], sh["p"], METRICS[metric], np.full(prior.shape, zero))
        assert bits_equal(got, want), (name, metric, zero)


@pytest.mark.parametrize("name", ir.DISCRIMINATING)
def test_restatement_equals_the_brute_force(name):
    """log-sum in numpy.longdouble against sum over c of P(c) exp(-d / 2 sigma^2) with P(c) = prod sigmoid(+-prior); two label bits
    unclaimed; the prior must matter on these layouts (it moves the LLRs by more than 1), so a sign or bit-order error is O(1)"""
    sh, src, rx, prior = ir.brute_case(name)
    assert np.finfo(np.longdouble).nmant >= 63
    m, L = sh["m"], sh["L"]
    tinv = ir.claims(src, L, m)
    assert (tinv < 0).sum() >= 2                                              # unclaimed label bits
    got, _ = ir.demod_prior(sh["points"], src, rx, 0.4, sh["N"], sh["p"], ir.LOGSUM, prior, np.longdouble)
    want = ir.brute_force(sh["points"], src, rx, 0.4, sh["N"], sh["p"], prior)
    without, _ = ir.demod_prior(sh["points"], src, rx, 0.4, sh["N"], sh["p"], ir.LOGSUM, np.zeros_like(prior), np.longdouble)
    err = float((np.abs(got - want) / np.maximum(1, np.abs(want))).max())
    print(f"{name}: worst |restatement - brute force| / max(1, |L|) = {err:.3e} (recorded {ir.BRUTE_FORCE_ERR:.3e}, bound {ir.BRUTE_FORCE_TOL:.3e}); "
          f"largest |L| {float(np.abs(want).max()):.1f}, the prior moves the LLRs by up to {float(np.abs(got - without).max()):.1f}")
    assert float(np.abs(got - without).max()) > 1.0
    assert err <= ir.BRUTE_FORCE_TOL


def within(got, want, scale, eps, what):
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble))
    ratio = float((err / np.where(scale > 0, scale, 1.0)).max())
    print(f"{what}: worst error / scale = {ratio / 2.0 ** -53:.3f} units of 2^-53 (bound {eps / 2.0 ** -53:.1f})")
    return bool((err <= eps * scale).all())


def test_anchor_aligned_gray_16qam():
    """gf64_16qam: a point is shared by two symbols, one owns the two in-phase label bits and the other the two quadrature bits (or
    the reverse).  d_s(c) = dI(c_I) + dQ(c_Q), so the foreign axis and its prior are one term common to every a: the prior cancels.
    Max-log in float64 within the derived bound; log-sum in float64 within ir.LOGSUM_TOL, in longdouble within the derived bound."""
    sh, rx, prior = ir.kernel_case("gf64_16qam")
    args = (sh["points"], sh["src"], rx, ir.KERNEL_SIGMA, sh["N"], sh["p"])
    eps = ir.anchor_eps(sh["m"])
    want, _ = dg.demod(*args, dg.MAXLOG)
    got, scale = ir.demod_prior(*args, ir.MAXLOG, prior)
    assert np.abs(prior).max() == 50.0 and within(got, want, scale, eps, "max-log")
    want_ls, _ = dg.demod(*args, dg.LOGSUM)
    got_ls, _ = ir.demod_prior(*args, ir.LOGSUM, prior)
    assert within(got_ls, want_ls, scale, ir.LOGSUM_TOL, "log-sum float64")
    want_ld, _ = dg.demod(*args, dg.LOGSUM, np.longdouble)
    got_ld, _ = ir.demod_prior(*args, ir.LOGSUM, prior, np.longdouble)
    assert within(got_ld, want_ld, scale, eps, "log-sum longdouble")
    assert not bits_equal(got_ls, want_ls)                                    # (the prior did enter the arithmetic)


def test_anchor_qpsk_straddling_is_two_bpsk_streams():
    """QPSK on (+-1, +-1), p = 3: every second point is shared by two symbols, one bit each; the foreign bit sits on the other axis,
    its term factorises and a prior on it cancels: the LLRs are those of BPSK on the interleaved real stream (Comm.cpp:356 +
    :364-378), whatever the prior"""
    N, p, B = 6, 3, 3
    points = np.array([[1.0, 1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, -1.0]])
    L = N * p // 2
    src = dg.src_table(N, p, (), 2, L)
    rng = np.random.default_rng(6)
    rx = points[rng.integers(0, 4, (B, L))] + 0.4 * rng.standard_normal((B, L, 2))
    prior = 4 * rng.standard_normal((B, N * p))
    prior[2] = 50.0 * (1 - 2 * rng.integers(0, 2, N * p))
    want = dg.bpsk_formula(src, rx.reshape(B, 2 * L), 0.4, N, p)
    got, scale = ir.demod_prior(points, src, rx, 0.4, N, p, ir.MAXLOG, prior)
    assert within(got, want, scale, ir.anchor_eps(2), "max-log")
    ls, _ = ir.demod_prior(points, src, rx, 0.4, N, p, ir.LOGSUM, prior)
    assert within(ls, want, scale, ir.LOGSUM_TOL, "log-sum float64")
    ld, _ = ir.demod_prior(points, src, rx, 0.4, N, p, ir.LOGSUM, prior, np.longdouble)
    assert within(ld, want, scale, ir.anchor_eps(2), "log-sum longdouble")
    assert not bits_equal(ls, got)                                            # a foreign bit: exp and log were evaluated


@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_host_layer_equals_the_restatement(name):
    """CComm::DemodulateGeneral with a prior: max-log bit for bit; log-sum within four times the float64 restatement's own error
    against the longdouble one on these inputs (floor dg.ANCHOR_EPS); prior = NULL IS the prior-less function"""
    sh, rx, prior = ir.kernel_case(name)
    args = (sh["N"], sh["p"], sh["points"], sh["src"], rx, ir.KERNEL_SIGMA)
    want, scale, _ = ir.kernel_want(name, ir.MAXLOG)
    got = hostlib.demod_general_prior(*args, ir.MAXLOG, prior)
    assert bits_equal(got, want) and np.isfinite(got).all()
    want_ls, scale, own = ir.kernel_want(name, ir.LOGSUM)
    print(f"{name}: float64 restatement against longdouble, worst error / scale = {own / 2.0 ** -53:.2f} units of 2^-53 "
          f"(recorded {ir.RESTATEMENT_LOGSUM_ERR / 2.0 ** -53:.1f})")
    assert own <= 1.25 * ir.RESTATEMENT_LOGSUM_ERR                            # (the record is not stale; the slack is demod_general's)
    ls = hostlib.demod_general_prior(*args, ir.LOGSUM, prior)
    assert within(ls, want_ls, scale, ir.LOGSUM_TOL, f"{name} host log-sum")
    for metric in (ir.MAXLOG, ir.LOGSUM):
        assert bits_equal(hostlib.demod_general_prior(*args, metric, None), hostlib.demod_general(*args, metric))
        assert bits_equal(hostlib.demod_general_prior(*args, metric, np.zeros_like(prior)), hostlib.demod_general(*args, metric))
    if name != "gf16_qpsk_aligned":                                           # (aligned: no foreign position, a prior is inert)
        assert not bits_equal(got, hostlib.demod_general(*args, ir.MAXLOG))
    else:
        assert bits_equal(got, hostlib.demod_general(*args, ir.MAXLOG))


@pytest.mark.parametrize("cell", sorted(ir.LOOP_CELLS))
def test_loop_cells_hold_the_convergence_mix(oracle, cell):
    """a condition of tests/test_gpu_idd.py, not a measurement: per the oracle's loop every cell has frames that converge in pass 1,
    one or more in a later pass, two or more never; passes = 1 is the plain decode"""
    import pyoracle as po
    sh, rx, sigma, max_iter, (out, conv, its, used) = ir.loop_cell(cell)
    never = int((conv == 0).sum())
    by_pass = [int(((conv == 1) & (used == k)).sum()) for k in range(1, ir.LOOP_PASSES + 1)]
    print(f"{cell}: converged in pass 1 / 2 / 3: {by_pass}, never: {never}")
    assert ir.has_loop_mix(conv, used), (cell, by_pass, never)
    assert (used[conv == 0] == ir.LOOP_PASSES).all() and ((used >= 1) & (used <= ir.LOOP_PASSES)).all()
    # passes = 1: what one decode of the prior-less LLRs gives
    code, edges, graph = ir.oracle_graph(ir.LOOP_CELLS[cell][0])
    od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.EMS, max_iter, po.CANONICAL, fixed_iters=0, **ir.LOOP_EMS)
    one = ir.loop(od, graph, sh, rx, sigma, ir.MAXLOG, 1, ir.MAXLOG)
    L, _ = dg.demod(sh["points"], sh["src"], rx, sigma, sh["N"], sh["p"], dg.MAXLOG)
    for b in range(rx.shape[0]):
        r, o, it = od.decode(L[b])
        assert (one[1][b], one[2][b], one[3][b]) == (int(r), int(it), 1) and np.array_equal(one[0][b], o)
        if used[b] == 1:                                                      # and the frames the loop finished in pass 1 are those
            assert conv[b] == int(r) == 1 and np.array_equal(out[b], o)


def test_extrinsic_is_the_posterior_without_the_channel_term(oracle):
    """NBL_SOFT_EXTRINSIC restated: the sum of the c2v alone; it is not the a-posteriori bit LLR minus the channel's bit LLR"""
    import pyoracle as po
    import soft_ref as sr
    sh, rx, sigma, max_iter, _ = ir.loop_cell("il64_it3")
    code, edges, graph = ir.oracle_graph("gf64_16qam_interleaved")
    od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.EMS, max_iter, po.CANONICAL, fixed_iters=0, **ir.LOOP_EMS)
    L, _ = dg.demod(sh["points"], sh["src"], rx[:1], sigma, sh["N"], sh["p"], dg.MAXLOG)
    od.decode(L[0])
    c2v = od.state()[2]
    sym, bits = ir.extrinsic_bits(c2v, graph, code.q, ir.MAXLOG)
    assert sr.bits_equal(sym, sr.posterior(np.zeros_like(L[0]), c2v, graph)) and bits.shape == (sh["N"] * sh["p"],)
    post = sr.bit_marginals(sr.posterior(L[0], c2v, graph), sh["p"], sr.MAXLOG)
    chan = sr.bit_marginals(L[0], sh["p"], sr.MAXLOG)
    assert np.abs((post - chan) - bits).max() > 1e-3
