"""Synthetic graphs for the OSD tests: bit lengths, fields and rates that no shipped code has.

Every shipped code has n = N log2(q) a multiple of 64, p = 4 / 6 / 8 and rate 1/2.  SHAPES names graphs of tests/degree_util.py
::degree_code at the edges of what nbl_create_osd accepts (any n <= 1024, p = 2 .. 8, any full-rank R < n); shape() builds one
and ASSERTS the property its line states (n, n % 64, n_dist, k, LDS bytes) instead of trusting the table.

OSD needs [CRC rows; H_bit] of full row rank (the reference's elimination never ends otherwise).  The rank is computed here in
Python over GF(2), from nbldpc_amd.datafiles.gf_matrices(q) and with the matrix laid out as tests/osd_check.cpp lays it out (the
loader leaves the matrix of alpha^(q-2) at zero, so an edge with that coefficient is a zero block).  `python tests/osd_shapes.py`
tries the seeds of SEEDS in turn and prints, per shape, the first one that passes (`seed`) and the first one that fails
(`bad_seed`, for the refusal test); both are written into the table below.
"""
import functools
import math

import numpy as np

from degree_util import degree_code

SEEDS = range(9100, 9200)
LOW = (1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3, 6, 2, 2, 3, 7, 2, 2, 3, 8)   # the variable-degree cycle of the deg_all_* fixtures
ALL_CHK = (2, 3, 4, 5, 6, 7, 8)
CAP_LDS = 160464

# id -> q, M, check-degree cycle, variable-degree cycle, seed, bad_seed (or None), CRC length and rows, and `expect`: the
# properties the shape is in the table for (N always; n, n % 64, n_dist, k = n - R, LDS bytes where its line says so)
SHAPES = {
    # one word per row (n < 64)
    "one_word": dict(q=4, M=16, chk=(4, 5), var=(2, 2, 3), seed=9100, bad_seed=9109, expect=dict(N=31, n=62, words=1)),
    # padded sort to 128, ONE bit in word 1
    "just_over_64": dict(q=32, M=6, chk=(5, 6), var=(2, 3), seed=9100, bad_seed=None, expect=dict(N=13, n=65, npow=128, mod64=1)),
    # p = 3, n_dist == n, partial last word
    "gf8_odd": dict(q=8, M=17, chk=(5, 6), var=(2, 3), seed=9100, bad_seed=None, expect=dict(N=37, n=111, n_dist=111, mod64=47)),
    # p = 3, n_dist = n - 1 inside a partial word
    "gf8_trunc": dict(q=8, M=18, chk=(3, 4, 6), var=(2,), seed=9100, bad_seed=9110, expect=dict(N=39, n=117, n_dist=116, mod64=53)),
    # p = 7, n_dist = n - 1
    "gf128": dict(q=128, M=14, chk=(4, 5, 6), var=(2, 2, 3), seed=9100, bad_seed=None, expect=dict(N=29, n=203, n_dist=202)),
    # n_dist = 896 = 14 * 64: the last word holds one bit and keeps none of the winner's (the only such (N, q) with n <= 1024)
    "trunc_on_boundary": dict(q=8, M=150, chk=(4, 4, 5, 5), var=(2, 2, 2, 3), seed=9100, bad_seed=None, expect=dict(N=299, n=897, n_dist=896, mod64=1)),
    # padded sort to 1024, second slot of the order rotation with one element (x = 512)
    "just_over_512": dict(q=8, M=86, chk=(3, 5, 6), var=(2, 2, 3), seed=9100, bad_seed=9108, expect=dict(N=171, n=513, npow=1024, mod64=1)),
    # the cap: LDS 160,464 B, rotation up to x = 1023
    "cap": dict(q=4, M=256, chk=(4,), var=(2,), seed=9112, bad_seed=9100, expect=dict(N=512, n=1024, lds=CAP_LDS)),
    # cap, partial word and n_dist = n - 1 at once
    "below_cap": dict(q=8, M=171, chk=(3, 4, 5, 6), var=(2, 2, 2, 3), seed=9101, bad_seed=9100, expect=dict(N=341, n=1023, n_dist=1022, mod64=63)),
    # k >> R: R = n / 8 (checks of degree 8 need variables of degree 1), G is most of the LDS
    "high_rate": dict(q=16, M=8, chk=(8,), var=(1,), seed=9100, bad_seed=None, expect=dict(N=64, n=256, k=224)),
    # R >> k: k = n / 8
    "low_rate": dict(q=16, M=56, chk=(3,), var=(3, 3, 2, 3, 3, 2, 3, 2), seed=9100, bad_seed=None, expect=dict(N=64, n=256, k=32)),
    # k = 1: N - M = 3 symbols of 3 bits, eight CRC-8 rows
    "k1": dict(q=8, M=9, chk=(3, 3, 2), var=(2,), seed=9101, bad_seed=9100, crc_len=8, crc_rows=8, expect=dict(N=12, n=36, k=1)),
    # k = 2: N - M = 1 symbol of 2 bits, no CRC rows.  (crc_len 2: the reference's CRC generator has (N - M) p - crc_len rows and
    # must have none here; nbl_create_osd looks at crc_len only when crc_rows > 0)
    "k2": dict(q=4, M=9, chk=(2, 2, 2, 2, 3, 2, 2, 2, 3), var=(2,), seed=9120, bad_seed=9100, crc_len=2, crc_rows=0, expect=dict(N=10, n=20, k=2)),
    # crc_rows < crc_len
    "crc16_rows5": dict(q=16, M=12, chk=(4,), var=(2,), seed=9100, bad_seed=None, crc_len=16, crc_rows=5, expect=dict(N=24, n=96, k=43)),
    "crc24_rows1": dict(q=32, M=10, chk=(4,), var=(2,), seed=9100, bad_seed=None, crc_len=24, crc_rows=1, expect=dict(N=20, n=100, k=49)),
    # checks of degree 2 - 8, variables of degree 1 - 8 under OSD
    "irregular": dict(q=16, M=14, chk=ALL_CHK, var=LOW, seed=9100, bad_seed=None, expect=dict(chk_degs=list(ALL_CHK), var_degs=[1, 2, 3, 4, 5, 6, 7, 8])),
}
CRC_PARTIAL = ("crc16_rows5", "crc24_rows1")
TRUNCATED = ("gf8_trunc", "trunc_on_boundary", "gf128", "below_cap")


def n_dist(N, q):
    """compute_min_distance_bit's CodeLen_bit: (int)(CodeLen * log(GFq) / log(2)), truncated from a double."""
    return int(N * math.log(q) / math.log(2))


def lds_bytes(n):
    """nbl_osd_lds_bytes, restated."""
    nw, npow = (n + 63) // 64, 1 << max(0, (n - 1).bit_length())
    return n * nw * 8 + n * 8 + npow * 12 + 5 * nw * 8 + 512 * 16 + 16 + 64


def _g_gauss(G, order):
    """G_GaussEliminate_bit as tests/osd_check.cpp::g_gauss states it, on a uint8 matrix."""
    rows, cols = G.shape
    row = 0
    while row < rows:
        col = order[row]
        if G[row, col] == 0:
            up = next((u for u in range(row + 1, rows) if G[u, col]), None)
            if up is not None:
                G[row] ^= G[up]
            else:
                order[row:] = order[row + 1:] + order[row:row + 1]
                row -= 1
        if row >= 0:
            for u in range(row + 1, rows):
                if G[u, col]:
                    G[u] ^= G[row]
        else:  # (the reference clears with row -1 here: it reads outside the matrix; the CRC generators never get there)
            raise AssertionError("rotation at row 0")
        row += 1
    for row in range(rows - 1, 0, -1):
        for u in range(row - 1, -1, -1):
            if G[u, order[row]] == 1:
                G[u] ^= G[row]


def osd_matrix(code, crc_len=8, crc_rows=0, gf_mat=None):
    """[CRC rows; H_bit] as uint8 [R][n], laid out as tests/osd_check.cpp (and the reference) lay it out."""
    import nbldpc_amd as nb
    q, N, M = code.q, code.N, code.M
    p = q.bit_length() - 1
    gm = nb.datafiles.gf_matrices(q) if gf_mat is None else gf_mat
    n, Mb = N * p, M * p
    msg = n - Mb
    H = np.zeros((Mb, n), dtype=np.uint8)
    e = 0
    for i in range(N):
        for _ in range(int(code.var_deg[i])):
            c, h = int(code.var_chk[e]), int(code.var_h[e])
            H[p * c:p * c + p, p * i:p * i + p] = np.asarray(gm[h]).T   # H[p c + k][p i + l] = gm[h][l][k]
            e += 1
    part = np.zeros((crc_rows, n), dtype=np.uint8)
    if crc_rows > 0:
        taps = {8: (0, 1, 4, 5, 7, 8), 16: (0, 4, 11, 16), 24: (0, 1, 18, 19, 23, 24)}[crc_len]
        G = np.zeros((msg - crc_len, msg), dtype=np.uint8)
        for i in range(msg - crc_len):
            G[i, [i + t for t in taps]] = 1
        _g_gauss(G, list(range(msg)))
        for i in range(crc_rows):
            part[i, :msg - crc_len] = G[:, msg - crc_rows + i]
            part[i, i + msg - crc_rows] = 1
    return np.concatenate([part, H], axis=0)


def gf2_rank(A):
    """Row rank over GF(2) of a 0/1 matrix (rows as Python integers)."""
    rows = [int("".join(map(str, r)), 2) if len(r) else 0 for r in np.asarray(A).tolist()]
    rank = 0
    while rows:
        piv = rows.pop()
        if piv:
            rank += 1
            low = piv & -piv
            rows = [r ^ piv if r & low else r for r in rows]
    return rank


def full_rank(code, crc_len=8, crc_rows=0, gf_mat=None):
    A = osd_matrix(code, crc_len, crc_rows, gf_mat)
    return A.shape[0] < A.shape[1] and gf2_rank(A) == A.shape[0]


def crc_of(name):
    s = SHAPES[name]
    return s.get("crc_len", 8), s.get("crc_rows", 0)


def build(name, seed):
    s = SHAPES[name]
    return degree_code(s["q"], seed, s["chk"], s["var"], s["M"])


@functools.lru_cache(maxsize=None)
def shape(name):
    """(nb.Code, oracle edge tuple, spec, info) of a named shape; info: n, p, R, k, n_dist, nw, npow, lds, crc_len, crc_rows.
    The properties the table states are asserted, and so is the rank."""
    s = SHAPES[name]
    code, edges, spec = build(name, s["seed"])
    crc_len, crc_rows = crc_of(name)
    p = s["q"].bit_length() - 1
    n = code.N * p
    R = code.M * p + crc_rows
    info = dict(n=n, p=p, R=R, k=n - R, n_dist=n_dist(code.N, s["q"]), nw=(n + 63) // 64, npow=1 << (n - 1).bit_length(), lds=lds_bytes(n),
                crc_len=crc_len, crc_rows=crc_rows, msg=n - code.M * p)
    got = dict(N=code.N, n=n, mod64=n % 64, words=info["nw"], n_dist=info["n_dist"], k=info["k"], npow=info["npow"], lds=info["lds"],
               chk_degs=sorted(set(code.chk_deg.tolist())), var_degs=sorted(set(code.var_deg.tolist())))
    for key, want in s["expect"].items():
        assert got[key] == want, (name, key, got[key], want)
    assert n <= 1024 and 0 < info["k"] and code.N > code.M and info["msg"] >= crc_len, (name, info)
    assert info["n_dist"] in (n, n - 1), (name, info)
    assert full_rank(code, crc_len, crc_rows), (name, "[CRC rows; H_bit] is not of full row rank")
    return code, edges, spec, info


def zero_block_variables(code, gf_mat=None):
    """Variables whose every edge carries alpha^(q-2), the coefficient whose matrix the loader leaves at zero: their columns of
    H_bit are zero, so the elimination rotates the order when it meets one of them first."""
    import nbldpc_amd as nb
    gm = nb.datafiles.gf_matrices(code.q) if gf_mat is None else gf_mat
    zero = [h for h in range(1, code.q) if not gm[h].any()]
    if gf_mat is not None and not zero:      # the full set of matrices: no element has a zero block
        return []
    assert len(zero) == 1
    out, e = [], 0
    for i in range(code.N):
        d = int(code.var_deg[i])
        if all(int(h) == zero[0] for h in code.var_h[e:e + d]):
            out.append(i)
        e += d
    return out


def bpsk_llr_zero(rng, code, B, ebn0_db):
    """Symbol LLRs of the all-zero codeword over BPSK / AWGN in the rate-1/2 convention (as test_gpu_parity._bpsk_llr_zero)."""
    p = code.q.bit_length() - 1
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((B, code.N, p))) / sigma ** 2
    a = np.arange(1, code.q)
    mask = ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64)
    return bit @ mask.T


def fixture_frames(name):
    """The eight frames of a shape's osd_shape_* fixture: all-zero-codeword BPSK LLRs at noise levels from 0 to 4 dB, real-valued
    and free of ties.  Frame 6 has its last symbol scaled by 0.01 (its bits rank last, become parity positions and are re-encoded:
    on a truncated shape the winner's bit at n_dist then differs from the base word's in about every other such frame); frame 7
    has a variable whose columns of H_bit are all zero scaled by 0.001 (the elimination meets it first and rotates the order at
    num_temp = n - 1), or variable 0 where the graph has none."""
    code, _, _, _ = shape(name)
    rng = np.random.default_rng(77000 + sorted(SHAPES).index(name))
    L = np.concatenate([bpsk_llr_zero(rng, code, 1, e) for e in (0.0, 0.0, 2.0, 2.0, 4.0, 4.0, 1.0, 3.0)], axis=0)
    L[6, -1] *= 0.01
    L[7, (zero_block_variables(code) or [0])[0]] *= 0.001
    return L


# Eb/N0 (dB, rate-1/2 convention) of the real-valued frames of the GPU tests, two frames each.  Chosen on the CPU with the oracle
# and the checker alone, so that EMS after 1 and after 2 iterations leaves converged and unconverged frames in every batch (a frame
# converges at iteration 1 only when its channel decisions are a codeword already: the last level) and the coverage conditions of
# tests/test_gpu_osd_shapes.py hold.
EBN0 = (0.0, 2.0, 5.0, 13.0)
FRAME_LABELS = ("real",) * 8 + ("weak_last", "weak_zero", "integer", "two_valued", "erased", "none_below_1e6", "just_below_1e6")
NONE_BELOW, JUST_BELOW = 13, 14
# seed of a shape's frames where 88000 + its index does not meet a condition.  k2: the only pair of information bits must win on
# some frame at order 2 (two flips with k = 2), else the `k >= 2` guard of the pair enumeration is not told apart from `k >= 3`;
# seeds tried from 88100 upwards, the first that passes assert_coverage
FRAME_SEEDS = {"k2": 88106}


def orders_of(name):
    """Orders 0 - 2 everywhere; 3 and 5 (which behaves as 3) where k <= 64."""
    return (0, 1, 2, 3, 5) if shape(name)[3]["k"] <= 64 else (0, 1, 2)


def gpu_frames(name, exe):
    """The 15 frames of a shape in the GPU tests (FRAME_LABELS): eight real-valued frames at EBN0; frame 0 with its last symbol
    scaled by 0.01 and frame 1 with an all-zero-column variable scaled by 0.001 (see fixture_frames); frame 0 rounded to integers,
    a two-valued frame and frame 2 with every third symbol erased (exact ties in the sort, exact-integer distances, equal integer
    parts); and frame 0 scaled so that its smallest candidate distance at the shape's largest order (from the checker's counters)
    is 1,000,000.5 -- every candidate at or above 1,000,000 (and far below 2^31), the smallest with the integer part 1,000,000 itself,
    which the reference's `distance < 1000000` still refuses -- and 999,999.5."""
    from osd_util import run_checker
    code, _, _, _ = shape(name)
    crc_len, crc_rows = crc_of(name)
    rng = np.random.default_rng(FRAME_SEEDS.get(name, 88000 + sorted(SHAPES).index(name)))
    real = np.concatenate([bpsk_llr_zero(rng, code, 2, e) for e in EBN0], axis=0)
    weak_last, weak_zero = real[0].copy(), real[1].copy()
    weak_last[-1] *= 0.01
    weak_zero[(zero_block_variables(code) or [0])[0]] *= 0.001
    integer = np.round(real[0])
    two = np.where(rng.random(real[0].shape) < 0.8, -2.0, 3.0)
    erased = real[2].copy()
    erased[::3] = 0.0
    _, c = run_checker(exe, code, real[:1], max(o for o in orders_of(name) if o <= 3), 1, crc_len, crc_rows, counters=True)
    d0 = float(c["best"][0])
    assert 0 < d0 < 1e6, (name, d0)
    L = np.concatenate([real, np.stack([weak_last, weak_zero, integer, two, erased, real[0] * (1000000.5 / d0), real[0] * (999999.5 / d0)])])
    assert L.shape[0] == len(FRAME_LABELS) and np.abs(L).sum(axis=(1, 2)).max() < 2.0 ** 31
    return L


_CASES = {}


def case(name, exe):
    """Frames and the checker's answer (outputs, counters) per order of one shape, flag 1; cached for the module."""
    from osd_util import run_checker
    if name not in _CASES:
        code, edges, _, info = shape(name)
        crc_len, crc_rows = crc_of(name)
        L = gpu_frames(name, exe)
        chk = {o: run_checker(exe, code, L, o, 1, crc_len, crc_rows, counters=True) for o in orders_of(name)}
        _CASES[name] = dict(code=code, edges=edges, info=info, L=L, chk=chk, osd=dict(crc_len=crc_len, crc_rows=crc_rows))
    return _CASES[name]


def assert_coverage(name, c):
    """The coverage conditions of one shape, on the checker's counters alone."""
    info, chk = c["info"], c["chk"]
    top = max(o for o in chk if o <= 3)
    cnt = chk[top][1]
    assert (cnt["rotations"] > 0).any() and (cnt["repairs"] > 0).any(), (name, cnt["rotations"], cnt["repairs"])
    if name in ("just_over_512", "below_cap", "cap"):
        assert cnt["max_rot"].max() >= 512, (name, cnt["max_rot"])
    if name == "just_over_512":
        assert cnt["max_rot"].max() == info["n"] - 1
    assert any(chk[o][1]["differs"].any() for o in chk if o >= 1), name
    if name in TRUNCATED:
        assert any(chk[o][1]["nd_bit"].any() for o in chk), (name, "no winner whose bit at n_dist differs from the base word's")
    for o in chk:
        assert chk[o][1]["flips"][NONE_BELOW] == -1 and chk[o][1]["best"][NONE_BELOW] >= 1e6, (name, o)
    assert chk[top][1]["best"][NONE_BELOW] < 1000001, (name, chk[top][1]["best"][NONE_BELOW])
    assert chk[top][1]["flips"][JUST_BELOW] >= 0 and 999999 <= chk[top][1]["best"][JUST_BELOW] < 1e6, (name, chk[top][1]["best"][JUST_BELOW])
    if info["k"] == 2:
        assert (chk[2][1]["flips"] == 2).any(), (name, "no frame whose winner flips both information bits")
    # exact ties reach the sort: the integer, two-valued and erased frames repeat reliabilities
    p, L = info["p"], c["L"]
    for b in (10, 11, 12):
        rel = np.abs(L[b][:, [(1 << k) - 1 for k in range(p)]]).reshape(-1)
        assert len(np.unique(rel)) < len(rel), (name, b)


if __name__ == "__main__":
    import sys
    for name in sys.argv[1:] or list(SHAPES):
        good = bad = None
        crc_len, crc_rows = crc_of(name)
        for seed in SEEDS:
            try:
                code, _, _ = build(name, seed)
            except AssertionError as e:
                print(name, seed, "no graph:", e)
                break
            ok = full_rank(code, crc_len, crc_rows)
            if ok and good is None and (name != "just_over_512" or zero_block_variables(code)):
                good = seed
            if not ok and bad is None:
                bad = seed
            if good is not None and (bad is not None or seed >= SEEDS[0] + 12):
                break
        print(f"{name}: N={code.N} seed={good} bad_seed={bad}", flush=True)
