"""The general demodulator of include/nbldpc.h (nbl_set_demodulator_ex) restated in numpy, for tests/test_demod_general.py (host
layer) and tests/test_gpu_demod_general.py (HIP kernel).  Nothing in the reference computes these LLRs, so what the new path rests on
is this restatement -- written as the header's formulas read, one Python loop per order the header fixes (points of a symbol
ascending, constellation indices ascending) -- and three anchors where it coincides with the two reference-pinned demodulators.

  demod(...)                the definition, float64 or numpy.longdouble; frames are the only vectorised axis
  puncture_modulate(...)    Puncture + Modulate (Comm.cpp:290-325) literally
  src_table(...)            the per-bit source table of the link chain: kept bit k -> label bit t = k, -1 beyond L m
  qary_formula / bpsk_formula   the two expressions of CComm::Demodulate (Comm.cpp:394-395, :356 + :364-378)
  shapes()                  the layouts both test files walk
"""
import numpy as np

LOGSUM, MAXLOG = 0, 1

# The three anchors, and force_general against the two existing kernels: every value must agree within
#   ANCHOR_EPS * scale,   scale = sum over the symbol's points s of (D_s(0) + D_s(a)) / (2 sigma^2)
# with the max-log D (at an aligned point D_s(x) is the distance d_s(x) itself).  Derivation: a distance (re-cr)*(re-cr) +
# (im-ci)*(im-ci) carries at most 4 rounding errors relative to its own size (two differences, two products; the sum of the two
# non-negative products adds none beyond its own); each of the two formulas compared puts one subtraction and one division on top,
# so together they stay under 16 units of 2^-53 relative to the scale: 2^-49.
ANCHOR_EPS = 2.0 ** -49

# Log-sum.  RESTATEMENT_LOGSUM_ERR is the worst error of the float64 restatement against the numpy.longdouble one, relative to the
# same scale, measured on the shapes and inputs of tests/test_gpu_demod_general.py (B = 3, sigma = 0.4, seed 11): 114.8 units of 2^-53,
# set by gf8_256qam (sums of up to 64 exponentials, and distances far below 2 sigma^2 log(sum)); every other shape stays under 6.
# The GPU is held to four times that, with a floor at ANCHOR_EPS: the factor covers a device exp / log of 1-2 ulp where libm's
# are correctly rounded in practice, and reductions of up to 128 terms.  DESIGN.md section 5e records both measured figures.
RESTATEMENT_LOGSUM_ERR = 1.275e-14
LOGSUM_TOL = max(4 * RESTATEMENT_LOGSUM_ERR, ANCHOR_EPS)


def demod(points, src, rx, sigma, N, p, metric, dtype=np.float64):
    """(L [B][N][q-1], scale [B][N][q-1]) of received samples rx [B][L][2]; points [M][2]; src [N p].  scale: see ANCHOR_EPS."""
    points = np.asarray(points, dtype=dtype)
    rx = np.asarray(rx, dtype=dtype)
    sigma = dtype(sigma)
    B, q, M = rx.shape[0], 1 << p, len(points)
    m = M.bit_length() - 1
    assert 1 << m == M
    two = dtype(2) * sigma * sigma
    out = np.zeros((B, N, q - 1), dtype=dtype)
    scale = np.zeros((B, N, q - 1), dtype=dtype)
    for n in range(N):
        ts = [int(src[n * p + j]) for j in range(p)]
        for s in sorted({t // m for t in ts if t >= 0}):                      # P(n), ascending
            owner = {t % m: j for j, t in enumerate(ts) if t >= 0 and t // m == s}   # label position -> bit of symbol n
            re, im = rx[:, s, 0], rx[:, s, 1]
            d = [(re - points[c, 0]) * (re - points[c, 0]) + (im - points[c, 1]) * (im - points[c, 1]) for c in range(M)]
            D, Dmin = {}, {}

            def metric_of(a):
                key = tuple((a >> j) & 1 for j in owner.values())
                if key not in D:
                    comp = [c for c in range(M) if all(((c >> (m - 1 - i)) & 1) == ((a >> j) & 1) for i, j in owner.items())]   # C_s(a)
                    dmin = d[comp[0]]
                    for c in comp[1:]:
                        dmin = np.minimum(dmin, d[c])
                    Dmin[key] = dmin
                    if metric == MAXLOG or len(comp) == 1:
                        D[key] = dmin
                    else:
                        total = np.zeros(B, dtype=dtype)
                        for c in comp:                                        # ascending c
                            total = total + np.exp(-(d[c] - dmin) / two)
                        D[key] = dmin - two * np.log(total)
                return D[key], Dmin[key]
            D0, M0 = metric_of(0)
            for a in range(1, q):
                Da, Ma = metric_of(a)
                out[:, n, a - 1] = out[:, n, a - 1] + (D0 - Da) / two
                scale[:, n, a - 1] += (M0 + Ma) / two
    return out, scale


def puncture_modulate(code_sym, p, punct, m, L):
    """Comm.cpp:255-325 for code words [B][N]: bits LSB first per symbol, the bits of the punctured symbols dropped, every m kept bits
    one constellation index, MSB first; the first L m kept bits only."""
    code_sym = np.asarray(code_sym)
    out = np.zeros((code_sym.shape[0], L), dtype=np.uint8)
    for b, word in enumerate(code_sym):
        code_bit = [(int(sym) >> k) & 1 for sym in word for k in range(p)]
        mod_bit = [x for i, x in enumerate(code_bit) if i // p not in punct]
        for s in range(L):
            idx = 0
            for k in range(m):
                idx += mod_bit[s * m + k] << (m - 1 - k)
            out[b, s] = idx
    return out


def src_table(N, p, punct, m, L):
    """kept bit k -> t = k, -1 once k >= L m (the tail MOD_SYM_LEN's floor drops) and for the bits of a punctured symbol"""
    src, k = [], 0
    for n in range(N):
        for _ in range(p):
            if n in punct:
                src.append(-1)
            else:
                src.append(k if k < L * m else -1)
                k += 1
    return np.array(src, dtype=np.int32)


def qary_formula(points, src_sym, rx, sigma):
    """Comm.cpp:394-395: one point per code symbol, src_sym [N] (-1 = punctured)"""
    B, q = rx.shape[0], len(points)
    out = np.zeros((B, len(src_sym), q - 1))
    c0r, c0i = points[0]
    for n, s in enumerate(src_sym):
        if s < 0:
            continue
        re, im = rx[:, s, 0], rx[:, s, 1]
        for a in range(1, q):
            cr, ci = points[a]
            out[:, n, a - 1] = ((2 * re - c0r - cr) * (cr - c0r) + (2 * im - c0i - ci) * (ci - c0i)) / (2 * sigma * sigma)
    return out


def bpsk_formula(src_bit, real, sigma, N, p):
    """Comm.cpp:356 and :364-378: real [B][number of samples], src_bit [N p] (-1 = punctured)"""
    B, q = real.shape[0], 1 << p
    llr = [np.zeros(B) if s < 0 else -2 * real[:, s] / (sigma * sigma) for s in src_bit]
    out = np.zeros((B, N, q - 1))
    for n in range(N):
        for a in range(1, q):
            acc = np.zeros(B)
            for k in range(p):
                if a & (1 << k):
                    acc = acc + llr[n * p + k]
            out[:, n, a - 1] = acc
    return out


def qary_src(N, p, punct):
    """force_general with M = q: symbol n on its own point, bit j of the value = bit j of the index = label position p-1-j"""
    src, s = [], 0
    for n in range(N):
        if n in punct:
            src += [-1] * p
        else:
            src += [s * p + (p - 1 - j) for j in range(p)]
            s += 1
    return np.array(src, dtype=np.int32), s


def psk8():
    k = np.arange(8)
    return np.stack([np.cos(2 * np.pi * k / 8), np.sin(2 * np.pi * k / 8)], axis=1)


def named_points(name):
    import nbldpc_amd.datafiles as df
    if name == "PSK8":
        return psk8()
    return np.array([[x[1], x[2]] for x in sorted(df.constellation(name))], dtype=np.float64)


U16, U256 = "divsalar.UNBLDPC.128.64.GF.16", "divsalar.UNBLDPC.128.64.GF.256"
# name -> (q, graph: a shipped code's name or a tests/degree_util.py profile, constellation, punctured symbols, layout)
SHAPES = {
    "gf16_qpsk_aligned": (16, U16, "GRAY_QPSK", (5,), "chain"),        # two points per symbol, no foreign bit; symbol 5 punctured
    "gf64_16qam": (64, "dc2mix", "GRAY_16QAM", (), "chain"),           # own bits 4+2 / 2+4: every second point shared by two symbols
    "gf256_64qam": (256, U256, "GRAY_64QAM", (), "chain"),             # own bits 2 / 4 / 6; 21 points, the last two code bits unsent
    "gf8_256qam": (8, "dc2mix", "GRAY_256QAM", (), "chain"),           # a point spans three or four symbols: 5 or 6 foreign bits of 8
    "gf4_8psk": (4, "dc2mix", "PSK8", (), "chain"),                    # m = 3
    "gf64_16qam_interleaved": (64, "dc2mix", "GRAY_16QAM", (), "permuted"),   # a fixed random bit interleaver: a symbol on six points
}


def graph(name):
    """(nb.Code, spec or None) of a shape"""
    import nbldpc_amd as nb
    from degree_util import profile_code
    q, g = SHAPES[name][:2]
    if g in (U16, U256):
        return nb.Code(g), None
    code, _, spec = profile_code(g, q)
    return code, spec


def shape(name, N=None):
    """dict(q, p, N, M, m, L, points, src) of a shape; N is the graph's unless given"""
    q, g, cons, punct, layout = SHAPES[name]
    if N is None:
        N = graph(name)[0].N
    p = q.bit_length() - 1
    points = named_points(cons)
    M = len(points)
    m = M.bit_length() - 1
    L = (N - len(punct)) * p // m
    src = src_table(N, p, punct, m, L)
    if layout == "permuted":
        t = np.concatenate([np.arange(L * m), np.full(N * p - L * m, -1)]).astype(np.int32)
        src = np.random.default_rng(20260).permutation(t).astype(np.int32)
    return dict(q=q, p=p, N=N, M=M, m=m, L=L, points=points, src=src, punct=list(punct))


def samples(sh, B, sigma, seed):
    """random transmitted points plus noise: (rx [B][L][2], tx index [B][L])"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, sh["M"], (B, sh["L"]))
    return sh["points"][idx] + sigma * rng.standard_normal((B, sh["L"], 2)), idx
