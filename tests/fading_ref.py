"""Flat fading of include/nbldpc.h (nbl_decode_batch_samples_csi, nbl_decode_batch_samples_idd_csi, nbl_set_fading) restated in numpy --
TEST INFRASTRUCTURE ONLY, for tests/test_fading.py (CPU) and tests/test_gpu_fading.py (HIP kernels).  Nothing in the reference computes
any of this, so what the feature rests on is this restatement -- written as the header's formulas read, on top of tests/demod_general.py
and tests/idd_ref.py -- a probability-domain brute force in another expression order, and three anchors that tie the gain-aware paths
to the reference-pinned gain-less ones.

  faded(points, hr, hi)    the faded table: pr = hr cr - hi ci, pi = hr ci + hi cr
  demod(...)               the general demodulator with per-sample gains (and an optional prior), float64 or numpy.longdouble
  brute_force(...)         the same LLRs from probabilities, |y - h c|^2 from complex arithmetic
  qary_formula / bpsk_formula   the two reference expressions with gains
  loop(...)                the iterative-demapping loop with gains on the canonical oracle
  Rand                     CRand (Rand.cpp:17-37) in Python floats and this machine's libm: the draws of Channel_Rayleigh
  kernel_case / brute_case / loop_cell   the inputs both test files walk
"""
import functools
import math

import numpy as np

import demod_general as dg
import idd_ref as ir

LOGSUM, MAXLOG = dg.LOGSUM, dg.MAXLOG

# ---- tolerances ------------------------------------------------------------------------------------------------------------------
# Everything is relative to idd_ref's scale, computed here on the faded points: sum over the symbol's points s of
# (M_s(0) + M_s(a)) / (2 sigma^2) + 6 P_s.
#
# Anchors.  gain == (1, 0): pr = 1 * cr - 0 * ci and pi = 1 * ci + 0 * cr are cr and ci exactly (a product with 1 is exact, a product
# with 0 is a zero, adding or subtracting a zero changes no number), so every distance and every LLR equals the gain-less one as a
# number: compared with ==, which lets the sign of a zero differ.  A constant gain: the faded table is the same for every sample, the
# arithmetic behind it is the gain-less demodulator's on that table, operation for operation: bit-identical.  BPSK with a real positive
# gain g: z = g * re + 0 * im = g * re exactly: bit-identical to the gain-less expression on samples g * re.
#
# Log-sum.  FADED_LOGSUM_ERR is the worst error of the float64 restatement against the numpy.longdouble one, relative to the scale,
# measured on kernel_case() (the six layouts, B = 3, sigma = 0.4, seed 31: faded samples, gains of magnitude 0.03 .. 10 with one exactly
# (1, 0), priors as idd_ref.kernel_case), with and without the prior: 231.0 units of 2^-53, set by gf8_256qam (the same frame with and
# without the prior; sums of up to 64 exponentials whose points a small gain has drawn together, so that the distances sit far below
# 2 sigma^2 log(sum)); every other shape stays under 7.  The AWGN figure is 114.8 (demod_general.RESTATEMENT_LOGSUM_ERR): it is not
# reused here.  Host layer and GPU are held to four times the measured figure with the floor demod_general.LOGSUM_TOL has: the
# project's rule.  DESIGN.md section 5k records the figure.
FADED_LOGSUM_ERR = 2.565e-14
LOGSUM_TOL = max(4 * FADED_LOGSUM_ERR, dg.ANCHOR_EPS)

# Brute force: worst |log-sum restatement - brute force|, both in numpy.longdouble, over brute_case() (the four discriminating layouts
# cut down to a few symbols, B = 3, sigma = 0.4, faded samples, gains as above, priors 4 randn, two label bits unclaimed), relative to
# max(1, |L|): 2.28e-18 (gf256_64qam, where |L| reaches 560; gf64_16qam_interleaved 2.17e-18).  A sign, conjugation or bit-order error
# shows as O(1).  The test holds the restatement to four times the figure.
BRUTE_FORCE_ERR = 2.29e-18
BRUTE_FORCE_TOL = 4 * BRUTE_FORCE_ERR


# ---- the demodulators with gains ------------------------------------------------------------------------------------------------
def faded(points, hr, hi):
    """(pr [M][...], pi [M][...]) of table points [M][2] under gains hr, hi (arrays of one shape): the header's two expressions"""
    pr = [hr * points[c, 0] - hi * points[c, 1] for c in range(len(points))]
    pi = [hr * points[c, 1] + hi * points[c, 0] for c in range(len(points))]
    return pr, pi


def demod(points, src, rx, gain, sigma, N, p, metric, prior=None, dtype=np.float64):
    """(L [B][N][q-1], scale [B][N][q-1]) of samples rx [B][L][2] with gains gain [B][L][2]; prior [B][N p] or None.
    idd_ref.demod_prior with the distance to the faded point; without a prior no term is subtracted (demod_general.demod)."""
    points = np.asarray(points, dtype=dtype)
    rx = np.asarray(rx, dtype=dtype)
    gain = np.asarray(gain, dtype=dtype)
    sigma = dtype(sigma)
    B, q, M = rx.shape[0], 1 << p, len(points)
    m = M.bit_length() - 1
    assert 1 << m == M and gain.shape == rx.shape
    if prior is not None:
        prior = np.asarray(prior, dtype=dtype)
        assert prior.shape == (B, N * p)
    two = dtype(2) * sigma * sigma
    tinv = ir.claims(src, rx.shape[1], m)
    out = np.zeros((B, N, q - 1), dtype=dtype)
    scale = np.zeros((B, N, q - 1), dtype=dtype)
    for n in range(N):
        ts = [int(src[n * p + j]) for j in range(p)]
        for s in sorted({t // m for t in ts if t >= 0}):                      # P(n), ascending
            owner = {t % m: j for j, t in enumerate(ts) if t >= 0 and t // m == s}   # label position -> bit of symbol n
            re, im = rx[:, s, 0], rx[:, s, 1]
            pr, pi = faded(points, gain[:, s, 0], gain[:, s, 1])
            plain = [(re - pr[c]) * (re - pr[c]) + (im - pi[c]) * (im - pi[c]) for c in range(M)]
            foreign = [i for i in range(m) if i not in owner and tinv[s * m + i] >= 0] if prior is not None else []
            d = []
            for c in range(M):
                if prior is None:
                    d.append(plain[c])
                    continue
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


def brute_force(points, src, rx, gain, sigma, N, p, prior):
    """idd_ref.brute_force over the faded channel, in numpy.longdouble / clongdouble: the distance is |y - h c|^2 with y, h, c complex
    numbers -- the complex product and the modulus, another expression order than the header's."""
    ld, cld = np.longdouble, np.clongdouble
    rx, gain, prior, sigma = np.asarray(rx, dtype=ld), np.asarray(gain, dtype=ld), np.asarray(prior, dtype=ld), ld(sigma)
    pts = np.asarray(points, dtype=ld)
    cpts = pts[:, 0].astype(cld) + cld(1j) * pts[:, 1].astype(cld)
    y = rx[..., 0].astype(cld) + cld(1j) * rx[..., 1].astype(cld)
    h = gain[..., 0].astype(cld) + cld(1j) * gain[..., 1].astype(cld)
    B, q, M = rx.shape[0], 1 << p, len(pts)
    m = M.bit_length() - 1
    two = ld(2) * sigma * sigma
    tinv = ir.claims(src, rx.shape[1], m)
    out = np.zeros((B, N, q - 1), dtype=ld)
    for n in range(N):
        ts = [int(src[n * p + j]) for j in range(p)]
        for s in sorted({t // m for t in ts if t >= 0}):
            owner = {t % m: j for j, t in enumerate(ts) if t >= 0 and t // m == s}
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
                        dist = np.abs(y[:, s] - h[:, s] * cpts[c]) ** 2
                        total = total + prob * np.exp(-dist / two)
                    seen[key] = total
                S[a] = seen[key]
            for a in range(1, q):
                out[:, n, a - 1] += np.log(S[a]) - np.log(S[0])
    return out


def qary_formula(points, src_sym, rx, gain, sigma):
    """Comm.cpp:394-395 on the faded points of the symbol's sample: src_sym [N] (-1 = punctured)"""
    B, q = rx.shape[0], len(points)
    out = np.zeros((B, len(src_sym), q - 1))
    for n, s in enumerate(src_sym):
        if s < 0:
            continue
        re, im = rx[:, s, 0], rx[:, s, 1]
        pr, pi = faded(np.asarray(points, dtype=np.float64), gain[:, s, 0], gain[:, s, 1])
        for a in range(1, q):
            out[:, n, a - 1] = ((2 * re - pr[0] - pr[a]) * (pr[a] - pr[0]) + (2 * im - pi[0] - pi[a]) * (pi[a] - pi[0])) / (2 * sigma * sigma)
    return out


def bpsk_formula(src_bit, rx, gain, sigma, N, p):
    """Comm.cpp:356 with z = hr re + hi im in place of re, then :364-378: src_bit [N p] (-1 = punctured)"""
    B = rx.shape[0]
    z = gain[..., 0] * rx[..., 0] + gain[..., 1] * rx[..., 1]
    llr = [np.zeros(B) if s < 0 else -2 * z[:, s] / (sigma * sigma) for s in src_bit]
    out = np.zeros((B, N, (1 << p) - 1))
    for n in range(N):
        for a in range(1, 1 << p):
            acc = np.zeros(B)
            for k in range(p):
                if a & (1 << k):
                    acc = acc + llr[n * p + k]
            out[:, n, a - 1] = acc
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def gains(B, L, seed):
    """[B][L][2]: complex normals times 10^U(-1.5, 1) -- magnitudes from well below to well above 1 -- and sample (0, 0) exactly (1, 0)"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, L, 2)) * np.sqrt(0.5) * 10.0 ** rng.uniform(-1.5, 1.0, (B, L, 1))
    g[0, 0] = (1.0, 0.0)
    return g


def faded_samples(sh, B, sigma, seed):
    """(rx, gain, tx index): random transmitted points through random gains, plus noise"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, sh["M"], (B, sh["L"]))
    gain = gains(B, sh["L"], seed + 1)
    c = sh["points"][idx]
    rx = np.stack([gain[..., 0] * c[..., 0] - gain[..., 1] * c[..., 1], gain[..., 0] * c[..., 1] + gain[..., 1] * c[..., 0]], axis=-1)
    return rx + sigma * rng.standard_normal((B, sh["L"], 2)), gain, idx


KERNEL_B, KERNEL_SIGMA, KERNEL_SEED = 3, 0.4, 31


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """(shape, rx, gain, prior) of the kernel / host-layer comparison: priors as idd_ref.kernel_case (4 randn, a row of zeros, a row of +-50)"""
    sh = dg.shape(name)
    rx, gain, _ = faded_samples(sh, KERNEL_B, KERNEL_SIGMA, KERNEL_SEED)
    rng = np.random.default_rng(KERNEL_SEED + 2)
    prior = 4 * rng.standard_normal((KERNEL_B, sh["N"] * sh["p"]))
    prior[1] = 0.0
    prior[2] = 50.0 * (1 - 2 * rng.integers(0, 2, prior.shape[1]))
    assert np.abs(gain).min() < 0.05 and np.hypot(gain[..., 0], gain[..., 1]).max() > 3.0 and tuple(gain[0, 0]) == (1.0, 0.0)
    for x in (rx, gain, prior):
        x.setflags(write=False)
    return sh, rx, gain, prior


@functools.lru_cache(maxsize=None)
def kernel_want(name, metric, with_prior):
    """(float64 restatement, scale, worst float64-against-longdouble error / scale) of kernel_case(name)"""
    sh, rx, gain, prior = kernel_case(name)
    pr = prior if with_prior else None
    want, scale = demod(sh["points"], sh["src"], rx, gain, KERNEL_SIGMA, sh["N"], sh["p"], metric, pr)
    err = 0.0
    if metric == LOGSUM:
        ld, _ = demod(sh["points"], sh["src"], rx, gain, KERNEL_SIGMA, sh["N"], sh["p"], metric, pr, np.longdouble)
        err = float((np.abs(want - ld) / np.where(scale > 0, scale, 1.0)).max())
    want.setflags(write=False)
    scale.setflags(write=False)
    return want, scale, err


@functools.lru_cache(maxsize=None)
def brute_case(name):
    """(shape, src with two unclaimed label bits, rx, gain, prior) of a cut-down discriminating layout: B = 3, sigma = 0.4"""
    sh = dg.shape(name, N=ir.BRUTE_N[name])
    src = ir.with_unclaimed(sh["src"], 2, 3)
    rx, gain, _ = faded_samples(sh, 3, 0.4, 41)
    prior = 4 * np.random.default_rng(43).standard_normal((3, sh["N"] * sh["p"]))
    return sh, src, rx, gain, prior


# the two small shapes of the BPSK and q-ary expressions
def small_case(kind):
    """(N, p, points, src, rx, gain, sigma, punctured symbols) of the BPSK case (divsalar.UNBLDPC.128.64.GF.16) or the punctured
    q-ary case (tests/link_shapes.py, qary_gf8_punct): B = 3, sigma = 0.4, gains as gains()"""
    import link_shapes as ls
    rng = np.random.default_rng(51)
    if kind == "bpsk":
        import nbldpc_amd as nb
        N, p, punct = nb.Code(dg.U16).N, 4, ()
        points = dg.named_points("BPSK")
        L = N * p
        src = np.arange(L, dtype=np.int32)
    else:
        code, _, info = ls.shape("qary_gf8_punct")
        N, p, punct = code.N, info["p"], tuple(info["punct"])
        points = ls.points_of("qary_gf8_punct")
        L = info["L"]
        src = np.array([-1 if n in punct else n - sum(1 for x in punct if x < n) for n in range(N)], dtype=np.int32)
    gain = gains(3, L, 52)
    c = points[rng.integers(0, len(points), (3, L))]
    rx = np.stack([gain[..., 0] * c[..., 0] - gain[..., 1] * c[..., 1], gain[..., 0] * c[..., 1] + gain[..., 1] * c[..., 0]], axis=-1)
    rx = rx + 0.4 * rng.standard_normal((3, L, 2))
    return N, p, points, src, rx, gain, 0.4, punct


# ---- the loop with gains -----------------------------------------------------------------------------------------------------------
def loop(od, graph, sh, rx, gain, sigma, demod_metric, passes, soft_metric):
    """idd_ref.loop with the gain-aware demodulator in every pass: (out [B][N], converged [B], iters [B], passes_used [B])"""
    B, N, p, q = rx.shape[0], sh["N"], sh["p"], sh["q"]
    out = np.zeros((B, N), dtype=np.int32)
    conv, iters, used = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    live = list(range(B))
    prior = np.zeros((B, N * p))
    for k in range(1, passes + 1):
        L, _ = demod(sh["points"], sh["src"], rx[live], gain[live], sigma, N, p, demod_metric, None if k == 1 else prior[live])
        left = []
        for row, b in enumerate(live):
            r, o, it = od.decode(L[row])
            if r or k == passes:
                out[b], conv[b], iters[b], used[b] = o, int(r), int(it), k
            else:
                prior[b] = ir.extrinsic_bits(od.state()[2], graph, q, soft_metric)[1]
                left.append(b)
        live = left
        if not live:
            break
    return out, conv, iters, used


# The loop cell with gains: gf64_16qam_interleaved, EMS nm = 16 nc = 3, max_iter 3, both metrics max-log, passes = 3, B = 24: the
# all-zero word (points[0] on every sample) through per-sample Rayleigh gains (default_rng(LOOP_SEED), unit mean power) plus sigma *
# noise.  Per the oracle it holds frames that converge in pass 1, in a later pass and never (has_loop_mix, asserted in both test files):
# pass 1 / later / never = 18 / 2 (pass 2) / 4 at sigma 0.3, seed 8.  (Seed 7 at sigma 0.3 and both seeds at 0.15 .. 0.25 showed no frame
# converging in a later pass.)
LOOP_NAME, LOOP_MAX_ITER, LOOP_SIGMA, LOOP_SEED = "gf64_16qam_interleaved", 3, 0.3, 8


def loop_samples(sh, sigma=LOOP_SIGMA, seed=LOOP_SEED, B=ir.LOOP_B):
    rng = np.random.default_rng(seed)
    gain = rng.standard_normal((B, sh["L"], 2)) * np.sqrt(0.5)
    c = sh["points"][0]
    rx = np.stack([gain[..., 0] * c[0] - gain[..., 1] * c[1], gain[..., 0] * c[1] + gain[..., 1] * c[0]], axis=-1)
    rx = rx + sigma * rng.standard_normal((B, sh["L"], 2))
    rx.setflags(write=False)
    gain.setflags(write=False)
    return rx, gain


@functools.lru_cache(maxsize=None)
def loop_cell():
    """(shape, rx, gain, sigma, max_iter, (out, converged, iters, passes_used) of the oracle's loop), computed once"""
    import pyoracle as po
    po.build()
    sh = dg.shape(LOOP_NAME)
    code, edges, graph = ir.oracle_graph(LOOP_NAME)
    rx, gain = loop_samples(sh)
    od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.EMS, LOOP_MAX_ITER, po.CANONICAL, fixed_iters=0, **ir.LOOP_EMS)
    ref = loop(od, graph, sh, rx, gain, LOOP_SIGMA, MAXLOG, ir.LOOP_PASSES, MAXLOG)
    for x in ref:
        x.setflags(write=False)
    return sh, rx, gain, LOOP_SIGMA, LOOP_MAX_ITER, ref


# ---- CRand and the Rayleigh frame --------------------------------------------------------------------------------------------------
class Rand:
    """CRand (Rand.cpp:17-37) in Python floats (IEEE doubles) and this machine's libm through the math module: the same operations in
    the same order as nbldpc_amd/host/rand.h"""

    def __init__(self, state):
        self.ix, self.iy, self.iz = (int(x) for x in state)

    def uniform(self):
        self.ix = self.ix * 249 % 61967
        self.iy = self.iy * 251 % 63443
        self.iz = self.iz * 252 % 63599
        t = self.ix / 61967.0 + self.iy / 63443.0 + self.iz / 63599.0
        return t - int(t)

    def norm(self, mu, sigma):
        u1 = self.uniform()
        u2 = self.uniform()
        return mu + sigma * math.cos(2 * math.acos(-1.0) * u2) * math.sqrt(-2.0 * math.log(1.0 - u1))

    def state(self):
        return np.array([self.ix, self.iy, self.iz], dtype=np.uint32)


def rayleigh_frame(state, tx_points, sigma, coherence):
    """One frame of include/nbldpc.h's Rayleigh channel from generator state [3]: (rx [L][2], gain [L][2], state after the frame);
    tx_points [L][2] the transmitted constellation points"""
    r = Rand(state)
    L = len(tx_points)
    nblk = -(-L // coherence)
    S = math.sqrt(0.5)
    h = [(r.norm(0, S), r.norm(0, S)) for _ in range(nblk)]
    rx, gain = np.zeros((L, 2)), np.zeros((L, 2))
    for s in range(L):
        hr, hi = h[s // coherence]
        cr, ci = float(tx_points[s][0]), float(tx_points[s][1])
        nr = r.norm(0, sigma)
        ni = r.norm(0, sigma)
        rx[s] = ((hr * cr - hi * ci) + nr, (hr * ci + hi * cr) + ni)
        gain[s] = (hr, hi)
    return rx, gain, r.state()


def awgn_noise(state, L, sigma):
    """the 2 L normals Channel_AWGN draws from generator state [3]: [L][2]"""
    r = Rand(state)
    return np.array([(r.norm(0, sigma), r.norm(0, sigma)) for _ in range(L)])
