"""Codes whose last wave of checks is partly empty: the cells of tests/test_tail_groups.py (CPU) and tests/test_gpu_tail_groups.py.

Three check-node kernel families pack G checks of one codeword into a wave and give a codeword ceil(M / G) workgroups:
nbl_cn_small.hip (q = 4 / 8 / 16 / 32: G = 64 / q), nbl_cn_ems64.hip and nbl_cn_bp64.hip (q = 64: G = 4).  With M mod G != 0 the
last workgroup of every codeword holds groups without a check; every shipped code and every other synthetic graph of the suite
has M in {8, 12, 14, 64, 128, 256, 288}, so only q = 4 and q = 8 ever met such a wave, with one residue each.  Here M walks the
residues: every class 1 .. G-1 where G <= 4; 1, G/2, G-1 and one M < G where G is 8 or 16.

A cell is (family, q, M, fused, method).  Its graph has check degrees 3, 4, 5 side by side (the bp64 family: the (2, 4) ring, the
only shape that kernel takes) and variable degrees (2, 3) -- the fused iteration -- or (2, 3, 4) -- the same check-node kernel
behind the separate variable-node launch.  Graphs, frames and seeds are fixed; nothing here touches the device."""
import collections
import functools

import numpy as np

from degree_util import degree_code, ring_code

Cell = collections.namedtuple("Cell", "family q M fused method")

# family -> {q: (G, the M of its cells)}
FAMILIES = {
    "small": {4: (16, (5, 17, 24, 31)), 8: (8, (5, 9, 12, 15)), 16: (4, (5, 6, 7)), 32: (2, (5, 7))},
    "ems64": {64: (4, (5, 6, 7, 9))},
    "bp64": {64: (4, (5, 6, 7, 9))},
}
# T-EMS stops at q = 32 and log-QSPA has no cell in the ems64 family: on an irregular GF(64) graph T-EMS runs the general kernel and
# log-QSPA the small-field kernel with G = 1, one check per workgroup either way -- no packed last wave.  The bp64 kernel is log-QSPA's.
FAMILY_METHODS = {"small": ("ems", "ems_plain", "tems", "bp"), "ems64": ("ems", "ems_plain"), "bp64": ("bp",)}
FAMILY_FUSED = {"small": (True, False), "ems64": (True, False), "bp64": (True,)}   # (the ring's unfused run is kernel variant 2)
CHK_DEGS = (3, 4, 5)
VAR_DEGS = {True: (2, 3), False: (2, 3, 4)}

METHOD_EMS, METHOD_TEMS, METHOD_BP = 2, 4, 1        # NBL_METHOD_* of include/nbldpc.h; oracle/pyoracle.py uses the same numbers
STATE_ITERS = {"ems": 4, "ems_plain": 4, "tems": 4, "bp": 3}
LONG_ITERS = {"ems": 8, "ems_plain": 8, "tems": 8, "bp": 3}   # batch residues and the active list (log-QSPA: test_tail_groups.py says why 3)


def cells():
    return [Cell(fam, q, M, fused, method) for fam, qs in FAMILIES.items() for q, (_, Ms) in qs.items() for M in Ms
            for fused in FAMILY_FUSED[fam] for method in FAMILY_METHODS[fam]]


def cell_id(c):
    return f"{c.family}-gf{c.q}-M{c.M}-{'fused' if c.fused else 'unfused'}-{c.method}"


CELLS = cells()
# one cell per (family, fused / unfused, method): fixed iterations
FIXED_CELLS = [c for c in CELLS if (c.q, c.M) in {(16, 6), (64, 7)}]
# one fused graph per family: batch residues and the active list
BATCH_CELLS = [c for c in CELLS if c.fused and (c.family, c.q, c.M) in {("small", 16, 5), ("ems64", 64, 5), ("bp64", 64, 7)}
               and c.method != "ems_plain"]


def group_size(c):
    return FAMILIES[c.family][c.q][0]


def method_of(c):
    """(method number, parameters): those of test_gpu_parity.py::test_field_sizes_without_a_shipped_code"""
    q = c.q
    return {"ems": (METHOD_EMS, dict(ems_nm=min(q, 6), ems_nc=2, ems_factor=1.1, ems_offset=0.1)),
            "ems_plain": (METHOD_EMS, dict(ems_nm=min(q, 5), ems_nc=5, ems_factor=1.0, ems_offset=0.0)),
            "tems": (METHOD_TEMS, dict(tems_nr=2, tems_nc=3, tems_factor=1.0, tems_offset=0.0)),
            "bp": (METHOD_BP, dict())}[c.method]


def planned_kernel(c, variant):
    """The check-node kernel nbl_debug_plan must name for the cell under nbl_debug_force_generic = variant"""
    if variant == 1:
        return {"ems": "ems", "ems_plain": "ems", "tems": "tems", "bp": "bp"}[c.method]
    if c.family == "small":
        return {"ems": "ems_small", "ems_plain": "ems_small", "tems": "tems_small", "bp": "bp_small"}[c.method]
    return c.family


@functools.lru_cache(maxsize=None)
def graph(family, q, M, fused):
    """(nb.Code, oracle edge tuple) of the cells with this graph"""
    if family == "bp64":
        code = ring_code(q, M, 4)
        ev = np.repeat(np.arange(code.N, dtype=np.int32), code.var_deg)
        return code, (code.N, code.M, code.q, ev, code.var_chk.copy(), code.var_h.copy())
    seed = 9000 + 100 * q + 2 * M + (0 if fused else 1) + (5000 if family == "ems64" else 0)
    code, edges, _ = degree_code(q, seed, CHK_DEGS, VAR_DEGS[fused], M)
    return code, edges


def cell_graph(c):
    return graph(c.family, c.q, c.M, c.fused)


# Cells whose log-QSPA frames are drawn from another stream than the default: the default one gave a frame on which the two FP64
# restatements of the oracle part ways by more than rounding (tests/test_tail_groups.py::test_log_qspa_frames_are_well_conditioned),
# so the kernel has no single answer to be compared with there.  The bump moves the seed; the frame kinds stay.
SEED_BUMP = {}


def _rng(c, salt):
    return np.random.default_rng([salt, c.q, c.M, int(c.fused), sorted(STATE_ITERS).index(c.method),
                                  sorted(FAMILIES).index(c.family), SEED_BUMP.get((cell_id(c), salt), 0)])


def state_frames(c):
    """B = 9: one full XCD group of 8 codeword slots and one slot of a second group whose other 7 lie beyond the batch.  Frames 1 and
    5 are strongly negative: every symbol decides 0, the all-zero word's syndrome is zero, and under early exit those two codewords
    leave the kernels through done[b] from iteration 2 on while their neighbours stay.  Frame 2 sits on the integer grid (ties),
    frame 3 is all zero.  log-QSPA takes a narrow real-valued frame in place of the integer one: exact ties between symbols are
    broken by the last bit of an exp / log chain there (tests/test_gpu_degrees.py::test_degree_grid_vs_oracle)."""
    code, _ = cell_graph(c)
    rng = _rng(c, 1)
    L = rng.normal(-1.5, 3.0, (9, code.N, c.q - 1))
    L[1] = rng.normal(-12.0, 2.5, (code.N, c.q - 1))
    L[2] = rng.normal(-0.5, 1.0, (code.N, c.q - 1)) if c.method == "bp" else np.round(rng.normal(-1.0, 2.0, (code.N, c.q - 1)))
    L[3] = 0.0
    L[5] = rng.normal(-12.0, 2.5, (code.N, c.q - 1))
    return L


LEAVE_AT_ONCE = (1, 5)   # the strongly negative frames of state_frames


def bpsk_zero_llr(rng, N, q, B, ebn0_db):
    """Symbol LLRs of the all-zero codeword over BPSK / AWGN in the rate-1/2 convention (as test_gpu_parity.py::_bpsk_llr_zero)"""
    p = q.bit_length() - 1
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((B, N, p))) / sigma ** 2
    a = np.arange(1, q)
    mask = ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64)
    return bit @ mask.T


MIX_EBN0 = (-3.0, 0.0, 3.0, 8.0)


def mixed_frames(c, B):
    """B frames (17: batch residues, 24: the active list's tile) of the all-zero codeword, Eb/N0 cycling through MIX_EBN0 frame by
    frame, so that every prefix mixes frames that converge at once, late and never on these weak graphs"""
    code, _ = cell_graph(c)
    rng = _rng(c, 2 if B == 17 else 3)
    per = [bpsk_zero_llr(rng, code.N, c.q, (B + len(MIX_EBN0) - 1) // len(MIX_EBN0), e) for e in MIX_EBN0]
    return np.stack([per[b % len(MIX_EBN0)][b // len(MIX_EBN0)] for b in range(B)])


TILES, POLLS = 43, (1, 3)   # the active list: 43 x 24 = 1032 codewords, poll intervals


def assert_leave_and_stay(ref):
    """oracle_run of state_frames under early exit: the strongly negative frames converge at iteration 1, another frame goes on"""
    for b in LEAVE_AT_ONCE:
        assert ref[b][0] == 1 and ref[b][2] == 1 and not ref[b][1].any(), (b, ref[b][:3])
    assert any(not (r == 1 and it == 1) for b, (r, _, it, _) in enumerate(ref) if b not in LEAVE_AT_ONCE)


def assert_mix(ref):
    """oracle_run of mixed_frames: frames that converge at iteration 1, later, and never; the converged share strictly inside (0.05, 1)"""
    conv = [it for r, _, it, _ in ref if r]
    assert 1 in conv and max(conv) > 1 and len(conv) < len(ref), [(r, it) for r, _, it, _ in ref]
    assert 0.05 < len(conv) / len(ref) < 1.0


def still_iterating(ref, window):
    """codewords of the tile that a window of `window` iterations leaves on the active list"""
    return sum(1 for r, _, it, _ in ref if not (r and it <= window))


def assert_partly_filled_list(ref, iters):
    """The list after the first window is no multiple of 8 long, for every poll interval that is followed by a second window: that
    window's last XCD group has slots beyond the list.  (The batch itself, 1032 = 8 x 129, fills its groups; the batch residues
    are test_batch_residues' part.)"""
    assert TILES * len(ref) == 1032
    windows = [p for p in POLLS if p < iters]
    assert windows, (POLLS, iters)
    for p in windows:
        n_act = TILES * still_iterating(ref, p)
        assert n_act > 0 and n_act % 8 != 0, (p, n_act)


def oracle_run(oracle, c, L, iters, mode=None, fixed=0, state=True):
    """[(flag, decisions, iterations, (post, v2c, c2v) | None)] per frame from oracle/pyoracle.py; mode: CANONICAL unless given"""
    _, edges = cell_graph(c)
    meth, kw = method_of(c)
    od = oracle.Decoder(oracle.Code(edges=edges), oracle.GF(c.q), meth, iters, oracle.CANONICAL if mode is None else mode,
                        fixed_iters=fixed, **kw)
    ref = []
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        ref.append((r, o.copy(), it, [x.copy() for x in od.state()] if state else None))
    return ref
