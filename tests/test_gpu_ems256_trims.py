"""Wave-uniform bookkeeping of the GF(256) EMS kernel (nbl_cn_ems256.hip) that left the vector ALU -- what each item could break:

  * packed gather offsets: lane k of the gather holds the offsets of list entries k .. k+3 in one word, a trip of four entries
    reads ONE word and takes it apart on the scalar unit.  A field read from the wrong word or the wrong place shows where a trip
    starts at a position that is no multiple of four: behind an empty run, behind a run of 1, 2 or 3 entries beyond a multiple
    of four.  So the lists are crafted by RUN LENGTH (a run = the members of one slot: bit 0 and bit 7 of the check-domain
    symbol), at every compile-time nm and at run-time nm on every layout;
  * the rank-0 reductions of the four edges side by side, the lower bucket bound formed only in front of the histogram, and
    nd = 0 from four compares of the bounds beside rank 0: fixed-iteration decodes far past convergence, where the gate of the
    short lists is on -- real values, integer values with ties, rank 0 tied in several lanes (the FP64 fallback of the keyed
    maximum, and a bound beside rank 0 that EQUALS rank 0: the count by ballots must still run), a frame that never converges
    (gate off throughout) and a converged frame with widely spread values (gate on, the bounds leave more than nm entries: the
    full selection, and with it the lower bucket bound, is needed late).

Everything on divsalar.UNBLDPC.128.64.GF.256 (16 variables, 8 checks), a handful of frames per decode; message state (c2v, v2c,
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
    """One frame [N][q-1] whose nm best symbols fall into `runs` (lengths of the four runs, in list order) on one edge of every
    variable (a variable feeds two checks with different coefficients: `which` = 0 / 1 steers its first / second check), and the
    (check, position) pairs steered."""
    g = _graph()
    edges = {}
    for m, row in enumerate(g):
        for pos, (v, h) in enumerate(row):
            edges.setdefault(v, []).append((m, pos, h))
    L = np.zeros((len(edges), Q - 1))
    t_all = np.arange(Q)
    steered = []
    for v in range(len(edges)):
        m, pos, h = edges[v][which]
        steered.append((m, pos))
        chosen = []
        for k, n in enumerate(runs):
            chosen.extend(rng.choice(t_all[_klass(t_all) == k], n, replace=False).tolist())
        a = np.array([mul[inv[h]][t] for t in chosen], dtype=np.int64)  # t = h a
        vec = -rng.uniform(10.0, 30.0, Q)        # everything else far below symbol 0 (value 0), all different
        vec[a] = rng.uniform(5.0, 15.0, len(a))  # the chosen ones above it (a chosen symbol 0 keeps its 0: it is the last of the nm)
        L[v] = vec[1:]
    return L, sorted(steered)


def run_shapes(nm):
    """Run lengths (four runs, sum nm): every run empty once -- the other three 1, 2 and 3 entries beyond a multiple of four where
    nm allows it -- and one shape without an empty run whose first three runs end 1, 2 and 3 entries beyond a multiple of four."""
    def three(n):  # n entries on three runs, remainders 1, 2, 3 modulo four first
        r = [1, 2, 3] if n >= 6 else [1, 2, n - 3] if n >= 4 else [1, 1, n - 2]
        left, k = n - sum(r), 0
        while left >= 4:
            r[k % 3] += 4
            left -= 4
            k += 1
        r[2] += left
        return r
    shapes = []
    for empty in range(4):
        r = three(nm)
        r.insert(empty, 0)
        shapes.append(tuple(r))
    shapes.append((5, 2, 7, nm - 14) if nm >= 15 else (1, 2, 3, nm - 6) if nm >= 7 else (1, 1, 2, nm - 4))
    assert all(sum(s) == nm and min(s) >= 0 and max(s) <= 64 for s in shapes), shapes
    return shapes


def test_run_shapes():
    """The premise of the packed-offset cases, from the generator alone: at every nm a list with each run empty once, and runs of 1,
    2 and 3 entries beyond a multiple of four in front of another run."""
    for nm in NMS:
        shapes = run_shapes(nm)
        assert {s.index(0) for s in shapes if 0 in s} == {0, 1, 2, 3}
        if nm >= 7:
            assert any({1, 2, 3} <= {x % 4 for x in s[:3]} for s in shapes), (nm, shapes)


_BATCH = {}


def crafted_batch(nm):
    """[10][N][q-1]: every shape of run_shapes(nm), steering the first and the second check of every variable (together: every
    list of every check).  Built once per nm."""
    if nm not in _BATCH:
        mul, inv = (np.array(x) for x in df.gf_tables(Q))
        rng = np.random.default_rng(8800 + nm)
        g = _graph()
        frames = []
        for runs in run_shapes(nm):
            for which in (0, 1):
                L, steered = craft(rng, runs, mul, inv, which)
                for m, pos in steered:  # the inputs of iteration 1 are the channel vectors: the steered lists have the intended runs
                    v, h = g[m][pos]
                    assert run_lengths(np.concatenate([[0.0], L[v]]), h, nm, mul) == runs, (runs, m, pos)
                frames.append(L)
        _BATCH[nm] = np.stack(frames)
        _BATCH[nm].setflags(write=False)
    return _BATCH[nm]


def _oracle_dec(oracle, iters, **kw):
    N, M, q, ev, ec, eh = df.code_edges(CODE)
    return oracle.Decoder(oracle.Code(edges=(N, M, q, ev, ec, eh)), oracle.GF(q), oracle.EMS, iters, oracle.CANONICAL, fixed_iters=1, **kw)


_REF = {}


def reference(oracle, key, L, iters, kw):
    """Oracle results of a batch, computed once per key and shared: [(converged, iterations, decisions, post, v2c, c2v)]."""
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
    for b, (r, it, o, oP, oV, oC) in enumerate(ref):
        assert (conv[b], iters[b]) == (r, it) and np.array_equal(out[b], o), (tag, b)
        P, V, Cc = dec.read_state(b)
        assert np.array_equal(Cc, oC) and np.array_equal(V, oV) and np.array_equal(P, oP), (tag, b)


def _decode_and_compare(oracle, key, L, iters, nm, nc, unfused):
    kw = dict(ems_nm=nm, ems_nc=nc, ems_factor=1.0, ems_offset=0.0)
    ref = reference(oracle, key + (nm, nc), L, iters, kw)
    dec = nb.Decoder(nb.Code(CODE), nb.METHOD_EMS, iters, fixed_iters=1, **kw)
    if unfused:
        _force_generic(dec, 2)
    dec.record_state(True)
    _compare(dec, ref, L, key + (nm, nc, unfused))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    dec.close()
    assert (n_vn, n_cn) == ((iters, iters) if unfused else (0, iters)), "the intended instance ran"
    return ref


# compile-time nm: 8, 16, 32, 64; run-time nm: 5 (remainder shape), 7 (just below a compile-time layout), 24 (on the layout of 32),
# 33 (one past a compile-time layout), 48 (on the layout of 64)
NMS = (8, 16, 32, 64, 5, 7, 24, 33, 48)


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
@pytest.mark.parametrize("nc", [3, 2])
@pytest.mark.parametrize("nm", NMS)
def test_packed_offsets(oracle, nm, nc, unfused):
    """Three iterations on the crafted run lengths (iteration 1 walks the crafted lists, the later ones whatever they lead to)."""
    _decode_and_compare(oracle, ("packed",), crafted_batch(nm), 3, nm, nc, unfused)


def _bpsk_llr_zero(rng, N, B, ebn0_db):
    """Symbol LLRs of the all-zero codeword over BPSK / AWGN at rate 1/2."""
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((B, N, 8))) / sigma ** 2
    a = np.arange(1, Q)
    mask = ((a[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float64)
    return bit @ mask.T


PAST_ITERS = 12
F_REAL, F_INT, F_TIED, F_NEVER, F_SPREAD = slice(0, 6), slice(6, 9), slice(9, 11), 11, 12


def past_convergence_batch():
    """[13][N][q-1]:
    0-5   real-valued LLRs at 3 dB: zero syndrome within a few iterations, then the gate is on;
    6-8   the same kind rounded to integers: ties everywhere;
    9-10  rank 0 tied: every non-zero symbol at -20 (frame 10: -20, -21 or -22), but on every variable three symbols of
          different lanes at exactly 0.0, the value of symbol 0.  The decisions are all zero (the lowest symbol wins), the gate
          is on from iteration 2; at iteration 1 every edge has its maximum in four lanes (the FP64 fallback of the keyed
          maximum), and wherever such a tie lasts the bound beside rank 0 equals rank 0 and cannot lie below the threshold;
    11    -4 dB: never converges, the gate stays off;
    12    the all-zero codeword with every non-zero symbol spread evenly over [-30, -1]: zero syndrome at iteration 1, but an
          entry only falls out of the short lists when it lies below (worst single deviation of an output) - (best value beside rank
          0 of the other edges) ~ -30 + 1 -- next to none does, the lists would be longer than nm, and the full selection runs
          with the gate on."""
    if "past" not in _BATCH:
        N = nb.Code(CODE).N
        rng = np.random.default_rng(9100)
        L = np.zeros((13, N, Q - 1))
        L[F_REAL] = _bpsk_llr_zero(rng, N, 6, 3.0)
        L[F_INT] = np.round(_bpsk_llr_zero(rng, N, 3, 3.0))
        L[9] = -20.0
        L[10] = -20.0 - rng.integers(0, 3, (N, Q - 1))
        for f in (9, 10):
            for v in range(N):
                lanes = rng.choice(np.arange(1, 64), 3, replace=False)               # symbol a sits in lane (a & 127) >> 1; lane 0 holds symbol 0
                a = 2 * lanes + rng.integers(0, 2, 3) + 128 * rng.integers(0, 2, 3)  # any slot of the lane
                L[f, v, a - 1] = 0.0
        L[F_NEVER] = _bpsk_llr_zero(rng, N, 1, -4.0)[0]
        L[F_SPREAD] = -rng.uniform(1.0, 30.0, (N, Q - 1))
        L.setflags(write=False)
        _BATCH["past"] = L
    return _BATCH["past"]


@pytest.mark.parametrize("nm,nc,unfused", [(32, 3, False), (32, 2, False), (24, 3, False), (8, 3, False), (32, 3, True), (24, 2, True)])
def test_past_convergence(oracle, nm, nc, unfused):
    """12 fixed iterations: the scalar nd = 0 proof beside the count by ballots, the lower bucket bound formed late, the four-way
    reductions with tied keys."""
    L = past_convergence_batch()
    assert np.array_equal(L[F_INT], np.round(L[F_INT])) and np.array_equal(L[F_TIED], np.round(L[F_TIED]))
    assert ((L[F_TIED] == 0.0).sum(axis=2) == 3).all() and (L[F_SPREAD] < 0).all()
    ref = _decode_and_compare(oracle, ("past",), L, PAST_ITERS, nm, nc, unfused)
    conv = [r for r, *_ in ref]
    assert sum(conv[F_REAL]) >= 5 and all(conv[F_TIED]) and conv[F_SPREAD], "zero syndrome: the gate is on"
    assert not conv[F_NEVER], "one frame on which the gate stays off"
