"""The gather convolutions of the GF(256) EMS kernel (nbl_cn_ems256.hip, gather_conv) walk a list as four runs -- by bit 0 and
bit 7 of the entry's check-domain symbol -- four entries per trip and then the remainder one by one, over run ends that are
handed to the loops as scalar values.  Where such loops (and any software pipeline laid over them: DESIGN.md section 4, "Gather
loops") can go wrong is at the ends of the runs: an empty run, a run shorter than a trip, the hand-over to the next non-empty
run, the remainder, the last entry of the list.  So the shapes here are chosen by RUN LENGTH, not by size:

  * crafted channel vectors whose nm best symbols fall into prescribed runs on the lists the gathers walk (one iteration: a
    check's inputs are then the channel vectors of its four variables),
  * short lists (fixed-iteration decodes far past convergence: 0-3 entries per list) beside full ones,
  * ties (integer LLRs, an all-zero frame: the -inf padding entries of the short lists sit next to real ones),
  * the unfused instance.

Everything on divsalar.UNBLDPC.128.64.GF.256 (16 variables, 8 checks), at most 28 frames per decode; message state (c2v, v2c,
post), decisions, flags and iteration counts are compared bit for bit with the canonical oracle."""
import ctypes as C

import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df

pytestmark = pytest.mark.gpu

CODE = "divsalar.UNBLDPC.128.64.GF.256"
Q = 256


def _force_generic(dec, on):
    """0: default kernel choice; 1: generic kernels only; 2: specialised kernels without the fused iteration"""
    dec.lib.nbl_debug_force_generic.argtypes = [C.c_void_p, C.c_int32]
    assert dec.lib.nbl_debug_force_generic(dec.h, int(on)) == 0


def _graph():
    """Per check, in the order the kernel numbers a check's edges (the code's check rows): [(variable, h)] * 4."""
    c = df.codes()[CODE]
    return [[(v - 1, h) for v, h in row] for row in c["chk_rows"]]


def _klass(t):
    """Run of a check-domain symbol t in the list image: 0 = (bit 0, bit 7) clear, 1 = bit 7 only, 2 = bit 0 only, 3 = both."""
    t = np.asarray(t)
    return 2 * (t & 1) + ((t >> 7) & 1)


def run_lengths(vec, h, nm, mul):
    """Run lengths of the nm best entries of a q-vector (entry 0 = symbol 0) seen through an edge of coefficient h: value
    descending, higher variable-domain symbol first among equals (the reference's sort)."""
    a = np.lexsort((-np.arange(Q), -vec))[:nm]
    return tuple(np.bincount(_klass(mul[h][a]), minlength=4).tolist())


def craft(rng, runs, mul, inv, which):
    """One frame [N][q-1] whose nm best symbols fall into `runs` (lengths of the four runs, in list order) on the steering edge of
    every variable, and the (check, position) pairs steered.  A variable feeds two checks with different coefficients, so only one
    of its two lists can be prescribed in a frame: `which` = 0 / 1 takes the variable's first / second check.  (In this code a
    variable sits at the same position in both of its checks; position 2 is the list of the one-way gather, position 3 that of
    the three-way gather.)"""
    g = _graph()
    edges = {}
    for m, row in enumerate(g):
        for pos, (v, h) in enumerate(row):
            edges.setdefault(v, []).append((m, pos, h))
    N = len(edges)
    L = np.zeros((N, Q - 1))
    t_all = np.arange(Q)
    steered = []
    for v in range(N):
        assert len(edges[v]) == 2
        m, pos, h = edges[v][which]
        steered.append((m, pos))
        chosen = []
        for k, n in enumerate(runs):
            pool = t_all[_klass(t_all) == k]
            chosen.extend(rng.choice(pool, n, replace=False).tolist())
        a = np.array([mul[inv[h]][t] for t in chosen], dtype=np.int64)  # t = h a
        vec = -rng.uniform(10.0, 30.0, Q)       # everything else far below symbol 0 (value 0), all different
        vec[a] = rng.uniform(5.0, 15.0, len(a))  # the chosen ones above it (a chosen symbol 0 keeps its 0: it is the last of the nm)
        L[v] = vec[1:]
    return L, sorted(steered)


def crafted_cases(nm):
    cases = [tuple(nm if k == c else 0 for k in range(4)) for c in range(4)]
    cases += [(1, 0, 0, nm - 1), (3, 5, 7, nm - 15), (4, 4, 4, nm - 12)]
    if nm == 8:
        cases.append((2, 2, 2, 2))
    if nm == 4:
        cases = [(1, 1, 1, 1)]
    return [r for r in cases if min(r) >= 0]


def _compare(dec, od, L, tag):
    out, conv, iters = dec.decode(L)
    n_conv = 0
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        n_conv += r
        assert (conv[b], iters[b]) == (r, it) and np.array_equal(out[b], o), (tag, b)
        P, V, Cc = dec.read_state(b)
        oP, oV, oC = od.state()
        assert np.array_equal(Cc, oC) and np.array_equal(V, oV) and np.array_equal(P, oP), (tag, b)
    return n_conv


def _oracle_dec(oracle, iters, fixed=0, **kw):
    N, M, q, ev, ec, eh = df.code_edges(CODE)
    return oracle.Decoder(oracle.Code(edges=(N, M, q, ev, ec, eh)), oracle.GF(q), oracle.EMS, iters, oracle.CANONICAL, fixed_iters=fixed, **kw)


def _crafted_batch(nm, seed):
    mul, inv = df.gf_tables(Q)
    mul, inv = np.array(mul), np.array(inv)
    rng = np.random.default_rng(seed)
    g = _graph()
    frames, want = [], []
    for runs in crafted_cases(nm):
        covered = set()
        for which in (0, 1):
            L, steered = craft(rng, runs, mul, inv, which)
            # the inputs of iteration 1 are the channel vectors: the run lengths of the steered lists are the intended ones
            for m, pos in steered:
                v, h = g[m][pos]
                assert run_lengths(np.concatenate([[0.0], L[v]]), h, nm, mul) == runs, (runs, m, pos)
            covered.update(steered)
            frames.append(L)
            want.append(runs)
        assert covered == {(m, pos) for m in range(len(g)) for pos in range(4)}, "every list of every check, in one of the two frames"
    return np.stack(frames), want


@pytest.mark.parametrize("nm", [8, 16, 32, 64, 5, 12, 24, 48, 4])
def test_crafted_run_lengths(oracle, nm):
    """One iteration on frames whose gather lists have prescribed run lengths: all nm entries in one run (each of the four), (1, 0,
    0, nm-1), (3, 5, 7, nm-15), (4, 4, 4, nm-12), (2, 2, 2, 2) at nm = 8, every run of length 1 at run-time nm = 4 -- where the
    lengths exist at that nm.  nm = 8, 16, 32, 64 are the compile-time instances, the others run on the layout of the next power
    of two.  nc = 3, the fused kernel."""
    L, want = _crafted_batch(nm, 4000 + nm)
    kw = dict(ems_nm=nm, ems_nc=3, ems_factor=1.0, ems_offset=0.0)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, 1, fixed_iters=1, **kw)
    dec.record_state(True)
    _compare(dec, _oracle_dec(oracle, 1, fixed=1, **kw), L, ("crafted", nm, want))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    dec.close()
    assert (n_vn, n_cn) == (0, 1), "the fused kernel ran"


def test_crafted_run_lengths_unfused(oracle):
    """The same on the unfused instance of the kernel (separate variable-node launch, the check node reads v2c), nm = 16."""
    nm = 16
    L, want = _crafted_batch(nm, 4100)
    kw = dict(ems_nm=nm, ems_nc=3, ems_factor=1.0, ems_offset=0.0)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, 1, fixed_iters=1, **kw)
    _force_generic(dec, 2)
    dec.record_state(True)
    _compare(dec, _oracle_dec(oracle, 1, fixed=1, **kw), L, ("unfused", want))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    dec.close()
    assert (n_vn, n_cn) == (1, 1), "the unfused instance ran"


def _bpsk_llr_zero(rng, N, B, ebn0_db):
    """Symbol LLRs of the all-zero codeword over BPSK / AWGN at rate 1/2."""
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((B, N, 8))) / sigma ** 2
    a = np.arange(1, Q)
    mask = ((a[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float64)
    return bit @ mask.T


@pytest.mark.parametrize("nm", [32, 24])
def test_short_lists_and_full_lists(oracle, nm):
    """Fixed-iteration decodes: 40 iterations at 3 dB -- the frames converge within a few and then run on short lists of 0-3
    entries per edge (empty lists, lists that end inside the first run, odd and even lengths) -- and 8 iterations at 0 dB, where
    the lists of the frames that have not converged are full to the end."""
    N = nb.Code(CODE).N
    kw = dict(ems_nm=nm, ems_nc=3, ems_factor=1.0, ems_offset=0.0)
    for ebn0, its, B, seed in ((3.0, 40, 24, 51), (0.0, 8, 16, 52)):
        L = _bpsk_llr_zero(np.random.default_rng(seed + nm), N, B, ebn0)
        dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, its, fixed_iters=1, **kw)
        dec.record_state(True)
        n_conv = _compare(dec, _oracle_dec(oracle, its, fixed=1, **kw), L, ("short", nm, ebn0))
        _, (n_vn, n_syn, n_cn) = dec.last_timing()
        dec.close()
        assert (n_vn, n_cn) == (0, its), "the fused kernel ran"
        assert (n_conv >= B // 2) if ebn0 == 3.0 else (n_conv <= B // 2), (ebn0, n_conv, "3 dB: mostly short lists; 0 dB: mostly full ones")


@pytest.mark.parametrize("nm", [32, 24])
def test_ties_and_padding(oracle, nm):
    """Integer-valued LLRs (exact ties inside and at the end of the lists) and an all-zero frame, past convergence: the short
    lists' -inf padding entries sit next to real ones."""
    N = nb.Code(CODE).N
    rng = np.random.default_rng(60 + nm)
    L = np.zeros((5, N, Q - 1))
    L[1] = np.round(rng.normal(-12.0, 2.5, (N, Q - 1)))
    L[2] = np.round(rng.normal(-2.0, 3.0, (N, Q - 1)))
    L[3] = -1.0 - np.abs(np.round(rng.normal(0.0, 1.5, (N, Q - 1))))
    L[4] = np.round(_bpsk_llr_zero(rng, N, 1, 3.0)[0])
    kw = dict(ems_nm=nm, ems_nc=3, ems_factor=1.0, ems_offset=0.0)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, 6, fixed_iters=1, **kw)
    dec.record_state(True)
    n_conv = _compare(dec, _oracle_dec(oracle, 6, fixed=1, **kw), L, ("ties", nm))
    dec.close()
    assert n_conv >= 3, "converged frames (short lists) are part of the batch"
