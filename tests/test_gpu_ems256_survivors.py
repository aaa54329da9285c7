"""Past convergence the GF(256) EMS kernel (nbl_cn_ems256.hip) classifies a check by nd, the number of its edges on which more
than rank 0 survives the exact thresholds: with nd <= 1 no configuration outside conf(q,1) can matter and the check goes straight
to the emit stage; nd >= 2 runs the short-list code.  (A separate path for nd == 2 -- one pair convolution of the two surviving
edges for each of the two other outputs, six position pairs with their own rounding order -- was built, measured and dropped,
DESIGN.md section 7; the cases for it stay: they are the checks right next to the ones that are skipped.)  The product build does
not report the class a check took, so the inputs are built to produce every class:

  * the all-zero codeword, strongly polarised (every non-zero symbol at -LAM): zero syndrome at iteration 1, the gate is on from
    iteration 2;
  * on a chosen set of variables ONE competitor symbol at -DEL, DEL << LAM.  A check sees a competitor on as many edges as it has
    chosen variables; the sets are taken so that 0, 1, 2, 3 and 4 such edges occur, and two of them at every one of the six position
    pairs.  A lone competitor edge does not survive its threshold (the other two edges of every output are fully polarised), so
    0 and 1 competitor edges give nd = 0 and k >= 2 give nd = k: per decode of 6 iterations 1170 checks with nd = 0, 60 with
    nd = 2 (10 per pair), 40 with nd = 3, 10 with nd = 4 and the 256 ungated checks of iteration 1 -- counted once by the diagnostic
    build (tools/stamps.py's counters) for every variant and instance below;
  * the check messages are divided by ems_factor = 8, so that the iterated vectors keep that shape (with factor 1 the messages of
    the first iteration push everything but symbol 0 down by LAM, and no pair of competitors beats a single deviation any more):
    a competitor costs DEL + LAM / 7, everything else 8 LAM / 7, at every gated iteration;
  * three variants of the -LAM entries: exactly equal (ties at the thresholds), a seeded jitter, integer values.

Everything on divsalar.UNBLDPC.128.64.GF.256 (16 variables, 8 checks), 32 frames, 6 fixed iterations; message state (c2v, v2c,
post), decisions, flags and iteration counts are compared bit for bit with the canonical oracle.  A realistic mix (3 dB, 40
iterations, 24 frames) lets the classes alternate within one codeword from iteration to iteration."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df

pytestmark = pytest.mark.gpu

CODE = "divsalar.UNBLDPC.128.64.GF.256"
Q = 256
LAM, DEL = 48.0, 1.0
FACTOR = 8.0
ITERS = 6


def _force_generic(dec, on):
    """0: default kernel choice; 1: generic kernels only; 2: specialised kernels without the fused iteration"""
    dec.lib.nbl_debug_force_generic.argtypes = [C.c_void_p, C.c_int32]
    assert dec.lib.nbl_debug_force_generic(dec.h, int(on)) == 0


def _graph():
    """Per check, in the order the kernel numbers a check's edges (the code's check rows): [(variable, h)] * 4."""
    c = df.codes()[CODE]
    return [[(v - 1, h) for v, h in row] for row in c["chk_rows"]]


def competitor_sets():
    """32 sets of variables: every subset of the four variables of check 0, and of the last check."""
    g = _graph()
    sets = []
    for m in (0, len(g) - 1):
        for k in range(5):
            for pos in itertools.combinations(range(4), k):
                sets.append(frozenset(g[m][p][0] for p in pos))
    return sets


def competitor_positions(chosen):
    """Per check: the positions of its edges whose variable is in `chosen`."""
    return [tuple(p for p, (v, _) in enumerate(row) if v in chosen) for row in _graph()]


def crafted_frames(variant, seed=7100):
    """[32][N][q-1] channel vectors of the crafted classes (symbol 0 is the implicit 0)."""
    rng = np.random.default_rng(seed)
    sets = competitor_sets()
    N = len({v for row in _graph() for v, _ in row})
    L = np.full((len(sets), N, Q - 1), -LAM)
    if variant == "jitter":
        L -= rng.uniform(0.0, 2.0, L.shape)
    elif variant == "integer":
        L -= rng.integers(0, 3, L.shape).astype(np.float64)
    else:
        assert variant == "equal"
    for f, chosen in enumerate(sets):
        for v in sorted(chosen):
            L[f, v, rng.integers(0, Q - 1)] = -DEL
    return L


def test_every_class_is_in_the_batch():
    """From the graph alone (no GPU work, but it is the premise of the GPU cases below): over the batch a check has 0, 1, 2, 3 and
    4 competitor edges, and two competitor edges at every one of the six position pairs."""
    counts, pairs = set(), set()
    for chosen in competitor_sets():
        for pos in competitor_positions(chosen):
            counts.add(len(pos))
            if len(pos) == 2:
                pairs.add(pos)
    assert counts == {0, 1, 2, 3, 4}
    assert pairs == set(itertools.combinations(range(4), 2))
    for variant in ("equal", "jitter", "integer"):
        L = crafted_frames(variant)
        assert L.shape[0] <= 32 and (L < 0).all(), "all-zero decisions at iteration 1: zero syndrome, the gate is on from iteration 2"
        assert ((L == -DEL).sum(axis=2) <= 1).all() and (L[L != -DEL] <= -LAM).all(), "one competitor at most, everything else at or below -LAM"
    assert np.array_equal(crafted_frames("integer"), np.round(crafted_frames("integer")))


def _oracle_dec(oracle, iters, **kw):
    N, M, q, ev, ec, eh = df.code_edges(CODE)
    return oracle.Decoder(oracle.Code(edges=(N, M, q, ev, ec, eh)), oracle.GF(q), oracle.EMS, iters, oracle.CANONICAL, fixed_iters=1, **kw)


_REF = {}


def reference(oracle, key, L, iters, kw):
    """Oracle results of a batch, computed once per (inputs, nm, nc) and shared: [(converged, iterations, decisions, post, v2c, c2v)]."""
    if key not in _REF:
        od = _oracle_dec(oracle, iters, **kw)
        res = []
        for b in range(L.shape[0]):
            r, o, it = od.decode(L[b])
            res.append((r, it, o.copy()) + tuple(od.state()))
        _REF[key] = res
    return _REF[key]


def _compare(dec, ref, L, tag):
    out, conv, iters = dec.decode(L)
    n_conv = 0
    for b, (r, it, o, oP, oV, oC) in enumerate(ref):
        n_conv += r
        assert (conv[b], iters[b]) == (r, it) and np.array_equal(out[b], o), (tag, b)
        P, V, Cc = dec.read_state(b)
        assert np.array_equal(Cc, oC) and np.array_equal(V, oV) and np.array_equal(P, oP), (tag, b)
    return n_conv


@functools.lru_cache(maxsize=None)
def _frames(variant):
    L = crafted_frames(variant)
    L.setflags(write=False)
    return L


def _run_crafted(oracle, variant, nm, nc, unfused=False):
    L = _frames(variant)
    kw = dict(ems_nm=nm, ems_nc=nc, ems_factor=FACTOR, ems_offset=0.0)
    ref = reference(oracle, ("crafted", variant, nm, nc), L, ITERS, kw)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, ITERS, fixed_iters=1, **kw)
    if unfused:
        _force_generic(dec, 2)
    dec.record_state(True)
    n_conv = _compare(dec, ref, L, (variant, nm, nc, unfused))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    dec.close()
    assert n_conv == L.shape[0], "every frame has zero syndrome from iteration 1: the gate is on"
    assert (n_vn, n_cn) == ((ITERS, ITERS) if unfused else (0, ITERS)), "the intended instance ran"


@pytest.mark.parametrize("variant,nm,nc", [("equal", 32, 3), ("jitter", 32, 3), ("integer", 32, 3),
                                           ("jitter", 8, 3), ("equal", 8, 3), ("integer", 24, 3), ("jitter", 24, 3),
                                           ("jitter", 32, 2), ("equal", 32, 2), ("integer", 8, 2), ("jitter", 24, 2)])
def test_crafted_classes(oracle, variant, nm, nc):
    """Every class on the fused kernel: nm = 32 and 8 (compile-time instances), nm = 24 (run-time nm on the layout of 32),
    nc = 3 and 2."""
    _run_crafted(oracle, variant, nm, nc)


def test_crafted_classes_unfused(oracle):
    """The same on the unfused instance of the kernel (separate variable-node launch, the check node reads v2c)."""
    _run_crafted(oracle, "jitter", 32, 3, unfused=True)


def _bpsk_llr_zero(rng, N, B, ebn0_db):
    """Symbol LLRs of the all-zero codeword over BPSK / AWGN at rate 1/2."""
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((B, N, 8))) / sigma ** 2
    a = np.arange(1, Q)
    mask = ((a[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float64)
    return bit @ mask.T


@pytest.mark.parametrize("nm,nc", [(32, 3), (32, 2)])
def test_realistic_mix(oracle, nm, nc):
    """3 dB, 40 fixed iterations, 24 frames: the frames converge within a few iterations and then alternate between the classes
    from iteration to iteration."""
    N, B, its = nb.Code(CODE).N, 24, 40
    L = _bpsk_llr_zero(np.random.default_rng(7300), N, B, 3.0)
    kw = dict(ems_nm=nm, ems_nc=nc, ems_factor=1.0, ems_offset=0.0)
    ref = reference(oracle, ("mix", nm, nc), L, its, kw)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, its, fixed_iters=1, **kw)
    dec.record_state(True)
    n_conv = _compare(dec, ref, L, ("mix", nm, nc))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    dec.close()
    assert (n_vn, n_cn) == (0, its), "the fused kernel ran"
    assert n_conv >= B // 2, "mostly converged frames"
