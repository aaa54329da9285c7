"""Iterative demapping of include/nbldpc.h (nbl_decode_batch_samples_prior, nbl_soft_output_ex, nbl_decode_batch_samples_idd) restated
in numpy -- TEST INFRASTRUCTURE ONLY, for tests/test_idd.py (CPU) and tests/test_gpu_idd.py (HIP kernels).  Nothing in the reference
computes any of this, so what the feature rests on is this restatement -- written as the header's formulas read, on top of
tests/demod_general.py (the prior-less demodulator), tests/soft_ref.py (the soft output) and the canonical oracle (the decode) -- a
probability-domain brute force of the prior-aware demodulator, and two anchors where a prior must cancel.

  demod_prior(...)       the prior-aware general demodulator, float64 or numpy.longdouble; frames are the only vectorised axis
  brute_force(...)       the same LLRs from probabilities: P(c) = prod sigmoid(+-prior), sum over c of P(c) exp(-d / 2 sigma^2)
  extrinsic_bits(...)    NBL_SOFT_EXTRINSIC: soft_ref.posterior from the all-0.0 vector, then soft_ref.bit_marginals
  loop(...)              the loop around a decode of one codeword (the canonical oracle's, or any callable of the same form)
  loop_cell(...)         the cells both test files walk, their samples and their oracle results (computed once)
"""
import functools

import numpy as np

import demod_general as dg
import layered_ref as lr
import soft_ref as sr

LOGSUM, MAXLOG = dg.LOGSUM, dg.MAXLOG

# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# Everything below is relative to the scale demod_prior returns,
#     scale[n][a-1] = sum over the symbol's points s of (M_s(0) + M_s(a)) / (2 sigma^2) + 6 P_s,
# M_s(x) the smallest PLAIN distance d_s(c) over C_s(x) and P_s the sum of |prior| over the claimed foreign positions of s.  With a
# zero prior it is demod_general's scale.  Where it comes from: a distance d' = d - (2 sigma^2) A carries the 4 roundings of d (see
# demod_general.ANCHOR_EPS) and at most m + 1 more -- m - 1 additions of A (the first, to 0.0, is exact), the product, the
# subtraction -- each relative to at most T(c) = d(c) + (2 sigma^2) P_s.  The c a minimum is taken at, computed or true, has
# d'(c) <= d'(c0) for the plain minimiser c0, hence d(c) <= M + 2 (2 sigma^2) P_s and T(c) <= M + 3 (2 sigma^2) P_s; two metrics per
# term of the LLR, divided by 2 sigma^2: (M(0) + M(a)) / (2 sigma^2) + 6 P_s.
#
# Factorising anchors (a prior may change nothing beyond rounding): the prior-aware side has 4 + (m + 1) roundings per metric plus the
# subtraction and the division of the LLR, m + 7 units of 2^-53; the side it is compared with -- the prior-less restatement (6 units) or
# the BPSK expression (the remaining 10 of demod_general's 16) -- at most 10: m + 17 units together.


def anchor_eps(m):
    return (m + 17) * 2.0 ** -53


# Brute force: worst |log-sum restatement - brute force|, both in numpy.longdouble, over the instances of tests/test_idd.py
# (brute_case(): the four discriminating layouts cut down to a few symbols, B = 3, sigma = 0.4, priors 4 randn, two label bits
# unclaimed), relative to max(1, |L|): 3.14e-18 (gf8_256qam: sums of up to 64 products; |L| reaches 28.7 on gf256_64qam, and on these
# inputs the prior moves the LLRs by 2.9 to 11).  A sign or bit-order error shows as O(1).  The test holds the restatement to four times
# the figure.
BRUTE_FORCE_ERR = 3.15e-18
BRUTE_FORCE_TOL = 4 * BRUTE_FORCE_ERR

# Log-sum with a prior: worst error of the float64 restatement against the longdouble one, relative to the scale above, on the
# inputs of tests/test_gpu_idd.py (kernel_case(): the six layouts, B = 3, sigma = 0.4, seed 11, priors 4 randn with a row of zeros and
# a row of +-50): 114.8 units of 2^-53, set by gf8_256qam on its row of zeros -- the very figure and frame of
# demod_general.RESTATEMENT_LOGSUM_ERR; every other shape stays under 4.2.  Host layer and GPU are held to four times that with the
# floor demod_general.LOGSUM_TOL has: its rule, and here its value.
RESTATEMENT_LOGSUM_ERR = 1.275e-14
LOGSUM_TOL = max(4 * RESTATEMENT_LOGSUM_ERR, dg.ANCHOR_EPS)


# ---- the prior-aware demodulator ------------------------------------------------------------------------------------------------
def claims(src, L, m):
    """tinv [L m]: the code bit g with src[g] == t, -1 where nobody claims label bit t"""
    tinv = np.full(L * m, -1, dtype=np.int64)
    for g, t in enumerate(src):
        if t >= 0:
            tinv[int(t)] = g
    return tinv


def demod_prior(points, src, rx, sigma, N, p, metric, prior, dtype=np.float64):
    """(L [B][N][q-1], scale [B][N][q-1]); prior [B][N p] bit LLRs ln P(1) / P(0) per code bit.  demod_general.demod with d' for d."""
    points = np.asarray(points, dtype=dtype)
    rx = np.asarray(rx, dtype=dtype)
    prior = np.asarray(prior, dtype=dtype)
    sigma = dtype(sigma)
    B, q, M = rx.shape[0], 1 << p, len(points)
    m = M.bit_length() - 1
    assert 1 << m == M and prior.shape == (B, N * p)
    two = dtype(2) * sigma * sigma
    tinv = claims(src, rx.shape[1], m)
    out = np.zeros((B, N, q - 1), dtype=dtype)
    scale = np.zeros((B, N, q - 1), dtype=dtype)
    for n in range(N):
        ts = [int(src[n * p + j]) for j in range(p)]
        for s in sorted({t // m for t in ts if t >= 0}):                      # P(n), ascending
            owner = {t % m: j for j, t in enumerate(ts) if t >= 0 and t // m == s}   # label position -> bit of symbol n
            re, im = rx[:, s, 0], rx[:, s, 1]
            plain = [(re - points[c, 0]) * (re - points[c, 0]) + (im - points[c, 1]) * (im - points[c, 1]) for c in range(M)]
            foreign = [i for i in range(m) if i not in owner and tinv[s * m + i] >= 0]   # claimed foreign positions, ascending
            d = []
            for c in range(M):
                A = np.zeros(B, dtype=dtype)
                for i in foreign:
                    if (c >> (m - 1 - i)) & 1:
                        A = A + prior[:, tinv[s * m + i]]
                d.append(plain[c] - two * A)
            psum = np.zeros(B, dtype=dtype)
            for i in foreign:
                psum = psum + np.abs(prior[:, tinv[s * m + i]])
            D, Pmin = {}, {}

            def metric_of(a):
                key = tuple((a >> j) & 1 for j in owner.values())
                if key not in D:
                    comp = [c for c in range(M) if all(((c >> (m - 1 - i)) & 1) == ((a >> j) & 1) for i, j in owner.items())]   # C_s(a)
                    dmin, pmin = d[comp[0]], plain[comp[0]]
                    for c in comp[1:]:
                        dmin = np.minimum(dmin, d[c])
                        pmin = np.minimum(pmin, plain[c])
                    Pmin[key] = pmin
                    if metric == MAXLOG or len(comp) == 1:
                        D[key] = dmin
                    else:
                        total = np.zeros(B, dtype=dtype)
                        for c in comp:                                        # ascending c
                            total = total + np.exp(-(d[c] - dmin) / two)
                        D[key] = dmin - two * np.log(total)
                return D[key], Pmin[key]
            D0, M0 = metric_of(0)
            for a in range(1, q):
                Da, Ma = metric_of(a)
                out[:, n, a - 1] = out[:, n, a - 1] + (D0 - Da) / two
                scale[:, n, a - 1] += (M0 + Ma) / two + 6 * psum
    return out, scale


def brute_force(points, src, rx, sigma, N, p, prior):
    """The exact symbol LLRs under independent bit priors, from probabilities, in numpy.longdouble:
    P(bit = 1) = sigmoid(prior), P(bit = 0) = sigmoid(-prior) for a claimed foreign bit, 1/2 for an unclaimed one;
    S_s(a) = sum over c in C_s(a) of P(foreign bits of c) exp(-d_s(c) / 2 sigma^2);  L[n][a-1] = sum_s ln S_s(a) - ln S_s(0)."""
    ld = np.longdouble
    points, rx, prior, sigma = np.asarray(points, dtype=ld), np.asarray(rx, dtype=ld), np.asarray(prior, dtype=ld), ld(sigma)
    B, q, M = rx.shape[0], 1 << p, len(points)
    m = M.bit_length() - 1
    two = ld(2) * sigma * sigma
    tinv = claims(src, rx.shape[1], m)
    out = np.zeros((B, N, q - 1), dtype=ld)
    for n in range(N):
        ts = [int(src[n * p + j]) for j in range(p)]
        for s in sorted({t // m for t in ts if t >= 0}):
            owner = {t % m: j for j, t in enumerate(ts) if t >= 0 and t // m == s}
            re, im = rx[:, s, 0], rx[:, s, 1]
            S = np.zeros((q, B), dtype=ld)
            seen = {}
            for a in range(q):
                key = tuple((a >> j) & 1 for j in owner.values())
                if key not in seen:
                    total = np.zeros(B, dtype=ld)
                    for c in range(M):
                        if not all(((c >> (m - 1 - i)) & 1) == ((a >> j) & 1) for i, j in owner.items()):
                            continue
                        prob = np.ones(B, dtype=ld)
                        for i in range(m):
                            if i in owner:
                                continue
                            g = tinv[s * m + i]
                            if g < 0:
                                prob = prob * ld(0.5)
                            else:
                                sign = ld(1) if (c >> (m - 1 - i)) & 1 else ld(-1)
                                prob = prob / (ld(1) + np.exp(-sign * prior[:, g]))
                        dist = (re - points[c, 0]) ** 2 + (im - points[c, 1]) ** 2
                        total = total + prob * np.exp(-dist / two)
                    seen[key] = total
                S[a] = seen[key]
            for a in range(1, q):
                out[:, n, a - 1] += np.log(S[a]) - np.log(S[0])
    return out


def with_unclaimed(src, count, seed):
    """src with `count` transmitted code bits switched off: their label bits stay on the air, claimed by nobody"""
    src = np.array(src, copy=True)
    on = np.flatnonzero(src >= 0)
    src[np.random.default_rng(seed).choice(on, count, replace=False)] = -1
    return src


DISCRIMINATING = ("gf8_256qam", "gf4_8psk", "gf64_16qam_interleaved", "gf256_64qam")
BRUTE_N = {"gf8_256qam": 6, "gf4_8psk": 6, "gf64_16qam_interleaved": 4, "gf256_64qam": 3}


@functools.lru_cache(maxsize=None)
def brute_case(name):
    """(shape, src with two unclaimed label bits, rx, prior) of a cut-down discriminating layout: B = 3, sigma = 0.4"""
    sh = dg.shape(name, N=BRUTE_N[name])
    src = with_unclaimed(sh["src"], 2, 3)
    rx, _ = dg.samples(sh, 3, 0.4, 21)
    prior = 4 * np.random.default_rng(22).standard_normal((3, sh["N"] * sh["p"]))
    return sh, src, rx, prior


KERNEL_B, KERNEL_SIGMA, KERNEL_SEED = 3, 0.4, 11


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """(shape, rx, prior) of the kernel / host-layer comparison: the samples of tests/test_gpu_demod_general.py, priors 4 randn,
    row 1 all zeros, row 2 +-50"""
    sh = dg.shape(name)
    rx, _ = dg.samples(sh, KERNEL_B, KERNEL_SIGMA, KERNEL_SEED)
    rng = np.random.default_rng(KERNEL_SEED + 1)
    prior = 4 * rng.standard_normal((KERNEL_B, sh["N"] * sh["p"]))
    prior[1] = 0.0
    prior[2] = 50.0 * (1 - 2 * rng.integers(0, 2, prior.shape[1]))
    for x in (rx, prior):
        x.setflags(write=False)
    return sh, rx, prior


@functools.lru_cache(maxsize=None)
def kernel_want(name, metric):
    """(float64 restatement, scale, worst float64-against-longdouble error / scale) of kernel_case(name)"""
    sh, rx, prior = kernel_case(name)
    want, scale = demod_prior(sh["points"], sh["src"], rx, KERNEL_SIGMA, sh["N"], sh["p"], metric, prior)
    err = 0.0
    if metric == LOGSUM:
        ld, _ = demod_prior(sh["points"], sh["src"], rx, KERNEL_SIGMA, sh["N"], sh["p"], metric, prior, np.longdouble)
        err = float((np.abs(want - ld) / np.where(scale > 0, scale, 1.0)).max())
    want.setflags(write=False)
    scale.setflags(write=False)
    return want, scale, err


# ---- extrinsic soft output and the loop --------------------------------------------------------------------------------------------
def extrinsic_bits(c2v_vm, graph, q, metric, dtype=np.float64):
    """NBL_SOFT_EXTRINSIC of one codeword: (sym_llr [N][q-1], bit_llr [N p]) from its c2v [E][q-1] (variable-major)"""
    P = sr.posterior(np.zeros((graph.N, q - 1)), c2v_vm, graph)
    return P, sr.bit_marginals(P, q.bit_length() - 1, metric, dtype)


def oracle_decode(od):
    """the decode callable loop() takes, on a canonical oracle `od` (a pyoracle.Decoder under early exit): its decoder and its state"""
    def decode(L):
        r, o, it = od.decode(L)
        return int(r), o, int(it), od.state()[2]
    return decode


def loop(decode, graph, sh, rx, sigma, demod_metric, passes, soft_metric):
    """The loop of include/nbldpc.h around `decode`, a callable L_ch [N][q-1] -> (converged, out [N], iters, c2v [E][q-1] variable-major)
    of one codeword from zero messages, or a pyoracle.Decoder under early exit (then oracle_decode of it):
    (out [B][N], converged [B], iters [B], passes_used [B]).  Codewords are independent; the frames still unconverged share one call
    of the restatement per pass only because frames are its vectorised axis (elementwise arithmetic: the same values as one by one)."""
    if not callable(decode):
        decode = oracle_decode(decode)
    B, N, p, q = rx.shape[0], sh["N"], sh["p"], sh["q"]
    out = np.zeros((B, N), dtype=np.int32)
    conv, iters, used = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    live = list(range(B))
    prior = np.zeros((B, N * p))                                              # prior_1
    for k in range(1, passes + 1):
        if k == 1:                                                            # (the zero prior: d' = d exactly)
            L, _ = dg.demod(sh["points"], sh["src"], rx, sigma, N, p, demod_metric)
        else:
            L, _ = demod_prior(sh["points"], sh["src"], rx[live], sigma, N, p, demod_metric, prior[live])
        left = []
        for row, b in enumerate(live):
            r, o, it, c2v = decode(L[row])
            if r or k == passes:
                out[b], conv[b], iters[b], used[b] = o, int(r), int(it), k
            else:
                prior[b] = extrinsic_bits(c2v, graph, q, soft_metric)[1]
                left.append(b)
        live = left
        if not live:
            break
    return out, conv, iters, used


# The loop cells: the all-zero word (points[0] on every sample) plus sigma * default_rng(7) noise, B = 24, EMS nm = 16 nc = 3, both
# metrics max-log, passes = 3.  Per the oracle each holds frames that converge in pass 1, at least one that converges in a later pass
# and two or more that never do (has_loop_mix, asserted inside the tests); pass 1 / later / never as found with the oracle:
#   gf64_16qam_interleaved  max_iter 3  sigma 0.4    17 / 3 (pass 2)          / 4
#   gf64_16qam_interleaved  max_iter 2  sigma 0.5     4 / 1 (pass 3)          / 19
#   gf256_64qam             max_iter 3  sigma 0.27   13 / 1 (pass 2)          / 10
# gf8_256qam is left out of the loop grid: sigma 0.08 .. 0.14 showed no frame converging in a later pass.
LOOP_B, LOOP_PASSES, LOOP_EMS = 24, 3, dict(ems_nm=16, ems_nc=3)
LOOP_CELLS = {"il64_it3": ("gf64_16qam_interleaved", 3, 0.4), "il64_it2": ("gf64_16qam_interleaved", 2, 0.5), "gf256": ("gf256_64qam", 3, 0.27)}
# one T-EMS cell (nr = 2, nc = 3) on a graph with p * maxdc = 24 <= 32; the same samples as il64_it3.  No mix is asserted for it.
TEMS_CELLS = {"il64_tems": ("gf64_16qam_interleaved", 3, 0.4)}
LOOP_TEMS = dict(tems_nr=2, tems_nc=3)


def loop_samples(sh, sigma, B=LOOP_B):
    rx = sh["points"][0] + sigma * np.random.default_rng(7).standard_normal((B, sh["L"], 2))
    rx.setflags(write=False)
    return rx


def oracle_graph(name):
    """(nb.Code, oracle edge tuple, layered_ref.Graph) of a demod_general shape"""
    import pyoracle as po
    code, _ = dg.graph(name)
    # (N, M, q, edge_var, edge_chk, edge_h) in variable-major order: what pyoracle.Code takes
    edges = (code.N, code.M, code.q, np.repeat(np.arange(code.N, dtype=np.int32), code.var_deg), code.var_chk, code.var_h)
    return code, edges, lr.Graph(po.Code(edges=edges))


@functools.lru_cache(maxsize=None)
def loop_cell(cell):
    """(shape, rx, sigma, max_iter, (out, converged, iters, passes_used) of the oracle's loop), computed once"""
    import pyoracle as po
    po.build()
    name, max_iter, sigma = LOOP_CELLS[cell] if cell in LOOP_CELLS else TEMS_CELLS[cell]
    sh = dg.shape(name)
    code, edges, graph = oracle_graph(name)
    rx = loop_samples(sh, sigma)
    if cell in LOOP_CELLS:
        od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.EMS, max_iter, po.CANONICAL, fixed_iters=0, **LOOP_EMS)
    else:
        od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.TEMS, max_iter, po.CANONICAL, fixed_iters=0, **LOOP_TEMS)
    ref = loop(od, graph, sh, rx, sigma, MAXLOG, LOOP_PASSES, MAXLOG)
    for x in ref:
        x.setflags(write=False)
    return sh, rx, sigma, max_iter, ref


def has_loop_mix(conv, used):
    """a frame that converged in pass 1, one in a later pass, two or more that never converged"""
    c = [int(k) for f, k in zip(conv, used) if f]
    return 1 in c and any(k > 1 for k in c) and sum(1 for f in conv if not f) >= 2
