"""The iterative-demapping loop of include/nbldpc.h (nbl_decode_batch_samples_idd / nbl_decode_batch_resident_idd) on every decoder
kind -- TEST INFRASTRUCTURE ONLY, no device.  tests/test_idd_kinds.py puts on the cells below, without a GPU, the conditions a GPU cell
must meet; tests/test_gpu_idd_kinds.py runs the loop of every cell on the kernels and compares it with the reference made here (each
computed once per process, shared and read-only).

A cell names a kernel programme (what nbl_debug_plan says runs), a graph with its constellation layout, max_iter, sigma, the decoder's
keywords and the reference the loop is compared with:

  exact        EMS and T-EMS, every programme, both schedules: idd_ref.loop around the canonical oracle -- its decoder and state under
               flooding, its single-check entry point inside layered_ref / layered_tems_ref under the layered schedules.  BS-TEMS:
               the same loop around tests/bstems_check.cpp in its canonical mode, one codeword per run, whose state output gives the
               c2v (the checker tests/test_gpu_bstems.py holds the kernel to, bit for bit).  All four outputs bit for bit.
  float        log-QSPA and FHT, every programme, both schedules: the same loop around their FP64 restatements (bp_wide_ref,
               layered_bp_ref, fht_ref).  Not bit-exact; the project's statement (tests/test_gpu_layered_bp.py) is equality of
               decisions, flags and iteration counts where every decision has a margin above GAP_MIN = 1e-6.  reference() returns a cell's
               smallest decide gap over every iteration of every pass of every frame, per the restatement alone.
  composition  EMS with OSD: the CPU checker of OSD has no state hook; out_sym of the loop is pinned by the chain of public calls alone
               (tests/test_gpu_idd_kinds.py).  OSD changes out_sym only, so flags, iteration counts and passes of the OSD cell are
               still those of the oracle's EMS loop.

Frames follow idd_ref.loop_samples: the all-zero word plus sigma * default_rng(7) noise; passes = 3, both metrics max-log.  Every shape
has foreign label bits (q = 16 and q = 256 on Gray 64-QAM, q = 64 on bit-interleaved Gray 16-QAM), or the loop would be inert.

sigma of a cell is chosen on the CPU with the cell's reference alone: scan() below (python tests/idd_kinds_cases.py CELL SIGMA..).
COUNTS records, per cell, the frames that converge in pass 1 / in a later pass / never, which tests/test_idd_kinds.py recomputes.
Hard condition on every cell: a frame converges in pass 1 and two or more go into pass 2.  The full mix of idd_ref.has_loop_mix holds
on at least one cell of every row; the cells without a later-pass convergence are listed in NO_LATER with the range scanned."""
import functools
import sys

import numpy as np

import demod_general as dg
import idd_ref as ir
import layered_ref as lr

PASSES = 3
GAP_MIN = 1e-6                                                               # tests/test_layered_bp.py, tests/test_fht.py: the same figure
EMS16, EMS64, EMS256 = dict(ems_nm=8, ems_nc=3), dict(ems_nm=16, ems_nc=3), dict(ems_nm=12, ems_nc=3)
TEMS = dict(tems_nr=2, tems_nc=3)
TEMS2 = dict(tems_nr=2, tems_nc=2)                                          # where the oracle's T-EMS with three deviations takes 10 to 30 s per cell
BS = dict(bs_nm=4, bs_nc=2)
OSD = dict(osd_order=1, osd_flag=1)

# graph -> (q, constellation, layout)
GRAPHS = {
    "dc2mix64": (64, "GRAY_16QAM", "permuted"),       # the graph and layout of demod_general's gf64_16qam_interleaved: N = 14
    "ring16": (16, "GRAY_64QAM", "chain"),            # ring_code(q, RING_M[q], 4): every check of degree 4, every variable of degree 2
    "ring64": (64, "GRAY_16QAM", "permuted"),
    "ring256": (256, "GRAY_64QAM", "chain"),
    "wide64": (64, "GRAY_16QAM", "permuted"),         # degree_code(64, 92, *WIDE_DEGS): check degrees 9 .. 32, N = 88
    "wide256": (256, "GRAY_64QAM", "chain"),          # degree_code(256, 91, [9, 16, 32], [2, 3], 6): a four-wave workgroup
    "bds64": (64, "GRAY_16QAM", "permuted"),          # the shipped BDS.576.288.GF.64: N = 96, rate 1/2 (the wide programmes under switch 3)
}


# Checks of the ring codes.  On 64-QAM (6 label bits) 8 checks give N = 16 symbols of 4 or 8 bits: 64 or 128 code bits, of which the
# last 4 or 2 are not sent.  A symbol with an unsent bit has two equal channel LLRs, a decide gap of exactly 0, which no float kind
# may have; 9 checks give N = 18 and every bit is sent (72 = 12 * 6, 144 = 24 * 6).  GF(64) on 16-QAM: 96 = 24 * 4 with 8 checks.
RING_M = {16: 9, 64: 8, 256: 9}
WIDE64_SEED = 92                                                             # the graph of fht_wide_cases.py's wide-64


def _cell(row, kernel, graph, family, ref, max_iter, sigma, B=24, fused=False, schedule="flooding", variant=0, **kw):
    return dict(row=row, kernel=kernel, graph=graph, family=family, ref=ref, max_iter=max_iter, sigma=sigma, B=B, fused=fused,
                schedule=schedule, variant=variant, kw=kw)


# name -> cell.  family: ems | tems | bp | fht | bstems; kw: the keywords nb.Decoder and nb.binding.debug_plan take beyond the method.
# B is 24 except on the two bp_wide cells: the FP64 log-QSPA restatement (the oracle's O(dc q^2) check at degree 32) takes about 0.35 s
# per frame and iteration there, 16 and 33 s for 24 frames of 2 iterations; they run 12 and 8 frames of 2 iterations, so that the
# first GPU test that needs the reference waits a few seconds for it, not half a minute.
CELLS = {
    # ---- fused kernels under nbl_create (variant = nbl_debug_force_generic: 1 the general kernel, 2 the specialised one unfused)
    "ems_small": _cell("fused", "ems_small", "ring16", "ems", "exact", 3, 0.26, fused=True, **EMS16),
    "ems_small_v1": _cell("fused", "ems", "ring16", "ems", "exact", 3, 0.26, variant=1, **EMS16),
    "ems_small_v2": _cell("fused", "ems_small", "ring16", "ems", "exact", 3, 0.26, variant=2, **EMS16),
    "tems_small": _cell("fused", "tems_small", "ring16", "tems", "exact", 3, 0.26, fused=True, **TEMS),
    "tems_small_v1": _cell("fused", "tems", "ring16", "tems", "exact", 3, 0.26, variant=1, **TEMS),
    "tems_small_v2": _cell("fused", "tems_small", "ring16", "tems", "exact", 3, 0.26, variant=2, **TEMS),
    "bp_small": _cell("fused", "bp_small", "ring16", "bp", "float", 3, 0.26, fused=True),
    "bp_small_v2": _cell("fused", "bp_small", "ring16", "bp", "float", 3, 0.26, variant=2),
    "ems64": _cell("fused", "ems64", "ring64", "ems", "exact", 3, 0.35, fused=True, **EMS64),
    "ems64_v2": _cell("fused", "ems64", "ring64", "ems", "exact", 3, 0.35, variant=2, **EMS64),
    "tems64": _cell("fused", "tems64", "ring64", "tems", "exact", 3, 0.35, fused=True, **TEMS),
    "tems64_v1": _cell("fused", "tems", "ring64", "tems", "exact", 3, 0.35, variant=1, **TEMS),
    "tems64_v2": _cell("fused", "tems64", "ring64", "tems", "exact", 3, 0.35, variant=2, **TEMS),
    "bp64": _cell("fused", "bp64", "ring64", "bp", "float", 3, 0.35, fused=True),
    "bp64_v1": _cell("fused", "bp", "ring64", "bp", "float", 3, 0.35, variant=1),
    "bp64_v2": _cell("fused", "bp64", "ring64", "bp", "float", 3, 0.35, variant=2),
    "tems256": _cell("fused", "tems256", "ring256", "tems", "exact", 3, 0.19, fused=True, **TEMS2),
    "bp256": _cell("fused", "bp256", "ring256", "bp", "float", 3, 0.2, fused=True),
    # ---- layered kinds on the dc2mix GF(64) shape
    "ems_layered": _cell("layered", "ems_layered", "dc2mix64", "ems", "exact", 3, 0.5, schedule="greedy", **EMS64),
    "tems_layered": _cell("layered", "tems_layered", "dc2mix64", "tems", "exact", 3, 0.5, schedule="greedy", damped=True, **TEMS),
    "bp_layered": _cell("layered", "bp_layered", "dc2mix64", "bp", "float", 3, 0.5, schedule="greedy", bp=True),
    "fht_layered": _cell("layered", "fht_layered", "dc2mix64", "fht", "float", 3, 0.5, schedule="greedy", fht=True),
    # ---- other kinds on the same shape
    "fht": _cell("other", "fht", "dc2mix64", "fht", "float", 3, 0.4, fht=True),
    "bstems": _cell("other", "bstems", "dc2mix64", "bstems", "exact", 3, 0.3, **BS),
    "ems_osd": _cell("other", "ems", "dc2mix64", "ems", "composition", 3, 0.4, **EMS64, **OSD),
    "bp": _cell("other", "bp", "dc2mix64", "bp", "float", 3, 0.4),
    # ---- wide kinds on the degree-9..32 graphs: rate 76/88 (40/46 on GF(256)); no sigma gave a frame that converges in a later pass
    "ems_wide": _cell("wide", "ems_wide", "wide64", "ems", "exact", 3, 0.175, wide=True, **EMS64),
    "ems_wide_layered": _cell("wide", "ems_wide_layered", "wide64", "ems", "exact", 3, 0.185, schedule="greedy", wide=True, **EMS64),
    "tems_wide": _cell("wide", "tems_wide", "wide64", "tems", "exact", 3, 0.16, tems_wide=True, **TEMS2),
    "tems_wide_layered": _cell("wide", "tems_wide_layered", "wide64", "tems", "exact", 3, 0.175, schedule="greedy", tems_wide=True, **TEMS2),
    "bp_wide": _cell("wide", "bp_wide", "wide64", "bp", "float", 2, 0.15, B=12, bp_wide=True),
    "bp_wide_layered": _cell("wide", "bp_wide_layered", "wide64", "bp", "float", 2, 0.18, B=8, schedule="greedy", bp_wide=True),
    "fht_wide": _cell("wide", "fht_wide", "wide64", "fht", "float", 3, 0.175, fht=True),
    "fht_wide_layered": _cell("wide", "fht_wide_layered", "wide64", "fht", "float", 3, 0.185, schedule="greedy", fht=True),
    "ems_wide256": _cell("wide", "ems_wide", "wide256", "ems", "exact", 3, 0.09, wide=True, **EMS256),
    # ---- the wide programmes on the shipped GF(64) code (rate 1/2, switch 3: the wide programme at any check degree), where the row
    # finds its frames that converge in a later pass
    "ems_wide_bds": _cell("wide", "ems_wide", "bds64", "ems", "exact", 3, 0.33, variant=3, wide=True, **EMS64),
    "ems_wide_layered_bds": _cell("wide", "ems_wide_layered", "bds64", "ems", "exact", 3, 0.39, schedule="greedy", variant=3, wide=True, **EMS64),
    "tems_wide_layered_bds": _cell("wide", "tems_wide_layered", "bds64", "tems", "exact", 3, 0.33, schedule="greedy", variant=3, tems_wide=True, **TEMS2),
    "fht_wide_bds": _cell("wide", "fht_wide", "bds64", "fht", "float", 3, 0.33, variant=3, fht=True),
    "fht_wide_layered_bds": _cell("wide", "fht_wide_layered", "bds64", "fht", "float", 3, 0.36, schedule="greedy", variant=3, fht=True),
}
ROWS = ("fused", "layered", "other", "wide")

# cell -> (frames converging in pass 1, in a later pass, never), per the cell's reference
COUNTS = {
    "ems_small": (14, 2, 8), "ems_small_v1": (14, 2, 8), "ems_small_v2": (14, 2, 8),
    "tems_small": (11, 3, 10), "tems_small_v1": (11, 3, 10), "tems_small_v2": (11, 3, 10),
    "bp_small": (16, 1, 7), "bp_small_v2": (16, 1, 7),
    "ems64": (9, 3, 12), "ems64_v2": (9, 3, 12),
    "tems64": (7, 2, 15), "tems64_v1": (7, 2, 15), "tems64_v2": (7, 2, 15),
    "bp64": (11, 3, 10), "bp64_v1": (11, 3, 10), "bp64_v2": (11, 3, 10),
    "tems256": (8, 3, 13), "bp256": (18, 1, 5),
    "ems_layered": (21, 1, 2), "tems_layered": (17, 3, 4), "bp_layered": (20, 1, 3), "fht_layered": (20, 1, 3),
    "fht": (14, 4, 6), "bstems": (17, 1, 6), "ems_osd": (17, 3, 4), "bp": (14, 4, 6),
    "ems_wide": (10, 0, 14), "ems_wide_layered": (13, 0, 11), "tems_wide": (13, 0, 11), "tems_wide_layered": (13, 0, 11),
    "bp_wide": (9, 0, 3), "bp_wide_layered": (4, 0, 4), "fht_wide": (9, 0, 15), "fht_wide_layered": (14, 0, 10),
    "ems_wide256": (14, 0, 10),
    "ems_wide_bds": (6, 2, 16), "ems_wide_layered_bds": (13, 5, 6), "tems_wide_layered_bds": (13, 2, 9),
    "fht_wide_bds": (6, 3, 15), "fht_wide_layered_bds": (15, 6, 3),
}
# cell -> the sigma range scanned (steps of 0.03, and of 0.0025 to 0.01 across the waterfall; the EMS cells also at 2 and 6 iterations
# and on the graphs of seeds 91 and 93) without finding a frame that converges in a later pass.  All are cells of the degree-9..32
# graphs, of rate 76/88 and 40/46: from the sigma at which every frame converges in pass 1 to the sigma at which none does.  The
# extrinsic LLRs of so weak a code move the demodulator too little; the row's frames that converge later are those of the *_bds cells.
NO_LATER = {
    "ems_wide": (0.12, 0.27), "ems_wide_layered": (0.12, 0.27), "tems_wide": (0.16, 0.175), "tems_wide_layered": (0.17, 0.185),
    "bp_wide": (0.15, 0.24), "bp_wide_layered": (0.15, 0.24), "fht_wide": (0.12, 0.27), "fht_wide_layered": (0.12, 0.27),
    "ems_wide256": (0.06, 0.14),
}


# ---- graphs, shapes and samples -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(name):
    """(nb.Code, pyoracle.Code, pyoracle.GF, layered_ref.Graph) of a graph"""
    import nbldpc_amd as nb
    import pyoracle
    from degree_util import degree_code, ring_code
    from fht_wide_cases import WIDE_DEGS
    from test_layered import oracle_edges
    q = GRAPHS[name][0]
    if name == "dc2mix64":
        code = dg.graph("gf64_16qam_interleaved")[0]
    elif name.startswith("ring"):
        code = ring_code(q, RING_M[q], 4)
    elif name == "bds64":
        code = nb.Code("BDS.576.288.GF.64")
    elif name == "wide64":
        code = degree_code(64, WIDE64_SEED, *WIDE_DEGS)[0]
    else:
        code = degree_code(256, 91, [9, 16, 32], [2, 3], 6)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(q)[0]))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    return code, ocode, gf, g


@functools.lru_cache(maxsize=None)
def shape(name):
    """dict(q, p, N, M, m, L, points, src) of a graph's layout, as demod_general.shape makes it"""
    if name == "dc2mix64":
        return dg.shape("gf64_16qam_interleaved")
    q, cons, layout = GRAPHS[name]
    N = graph(name)[0].N
    p = q.bit_length() - 1
    points = dg.named_points(cons)
    M = len(points)
    m = M.bit_length() - 1
    L = N * p // m
    src = dg.src_table(N, p, (), m, L)
    if layout == "permuted":                                                  # demod_general.shape's fixed random bit interleaver
        src = np.random.default_rng(20260).permutation(src).astype(np.int32)
    return dict(q=q, p=p, N=N, M=M, m=m, L=L, points=points, src=src, punct=[])


def has_foreign_bits(sh):
    """some constellation point carries label bits of two code symbols"""
    owners = {}
    for g, t in enumerate(sh["src"]):
        if t >= 0:
            owners.setdefault(int(t) // sh["m"], set()).add(g // sh["p"])
    return any(len(v) > 1 for v in owners.values())


def samples(cell, sigma=None):
    c = CELLS[cell]
    return ir.loop_samples(shape(c["graph"]), c["sigma"] if sigma is None else sigma, c["B"])


def layer_of(cell):
    import nbldpc_amd as nb
    c = CELLS[cell]
    return None if c["schedule"] == "flooding" else nb.layer_greedy(graph(c["graph"])[0])


# ---- the decoder a cell describes ------------------------------------------------------------------------------------------------
def method_of(cell):
    import nbldpc_amd as nb
    return {"ems": nb.METHOD_EMS, "tems": nb.METHOD_TEMS, "bp": nb.METHOD_BP, "fht": nb.METHOD_BP, "bstems": nb.METHOD_BS_TEMS}[CELLS[cell]["family"]]


def plan(cell):
    """(kernel name, fusable, fused, want_v2c) of nb.binding.debug_plan for the cell's decoder"""
    import nbldpc_amd as nb
    c = CELLS[cell]
    kw = {k: v for k, v in c["kw"].items() if k not in OSD and k not in ("bp",)}
    if c["schedule"] != "flooding":
        kw["layers"] = "greedy"
    return nb.binding.debug_plan(graph(c["graph"])[0], method_of(cell), force_generic=c["variant"], **kw)


def decoder(cell, poll_every=0, **more):
    """the cell's nb.Decoder with its demodulator set (max-log) and its debug switch thrown; needs a device"""
    import ctypes as C
    import nbldpc_amd as nb
    c = CELLS[cell]
    sh = shape(c["graph"])
    kw = dict(c["kw"])
    if c["schedule"] != "flooding":
        kw["layers"] = "greedy"
    dec = nb.Decoder(graph(c["graph"])[0], method_of(cell), c["max_iter"], fixed_iters=0, poll_every=poll_every, **kw, **more)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
    if c["variant"]:
        dec.lib.nbl_debug_force_generic.argtypes = [C.c_void_p, C.c_int32]
        assert dec.lib.nbl_debug_force_generic(dec.h, c["variant"]) == 0
    return dec


# ---- references ----------------------------------------------------------------------------------------------------------------
def decode_callable(cell, schedule=None, gaps=None):
    """decode(L) -> (converged, out, iters, c2v variable-major) of the cell's reference from zero messages, one codeword; `gaps`: a list
    that receives the smallest decide gap of every call (float kinds).  schedule: the cell's unless given."""
    import pyoracle
    c = CELLS[cell]
    code, ocode, gf, g = graph(c["graph"])
    schedule = c["schedule"] if schedule is None else schedule
    import nbldpc_amd as nb
    lay = None if schedule == "flooding" else nb.layer_greedy(code)
    it = c["max_iter"]
    kw = {k: v for k, v in c["kw"].items() if k in ORACLE_KW}
    fam = c["family"]
    if fam == "ems":
        od = pyoracle.Decoder(ocode, gf, pyoracle.EMS, it, pyoracle.CANONICAL, fixed_iters=0, **kw)
        if lay is None:
            return ir.oracle_decode(od)

        def decode(L):
            out, r, n, _, c2v = lr.decode(od, gf.mul, L, lay, it)
            return int(r), out, int(n), c2v
        return decode
    if fam == "tems":
        import layered_tems_ref as ltr
        od = pyoracle.Decoder(ocode, gf, pyoracle.TEMS, it, pyoracle.CANONICAL, fixed_iters=0, **kw)
        if lay is None:
            return ir.oracle_decode(od)

        def decode(L):
            out, r, n, _, c2v = ltr.decode(od, gf.mul, L, lay, it)[:5]
            return int(r), out, int(n), c2v
        return decode
    if fam == "bp":
        import bp_wide_ref
        import layered_bp_ref as lbr
        od = pyoracle.Decoder(ocode, gf, pyoracle.BP, it, pyoracle.CANONICAL, fixed_iters=0)

        def decode(L):
            if lay is None:
                r = bp_wide_ref.decode_flooding(od, gf.mul, L, it)
                gap = r[6]
            else:
                r = lbr.decode(od, gf.mul, L, lay, it)
                gap = r[8]
            if gaps is not None:
                gaps.append(gap)
            return int(r[1]), r[0], int(r[2]), r[4]
        return decode
    if fam == "fht":
        import fht_ref
        chk = fht_ref.FhtCheck(ocode, gf.mul)

        def decode(L):
            r = fht_ref.decode(chk, L, lay, it)
            if gaps is not None:
                gaps.append(r[6])
            return int(r[1]), r[0], int(r[2]), r[4]
        return decode
    if fam == "bstems":
        from bstems_util import CANONICAL, run_checker
        exe = _bstems_checker()

        def decode(L):
            out, ret, its, st = run_checker(exe, code, L[None], it, CANONICAL, state=(0,), threads=1, **c["kw"])
            return int(ret[0] == 1), out[0].copy(), int(its[0]), st[0][2].copy()
        return decode
    raise ValueError(f"{cell}: unknown family {fam}")


@functools.lru_cache(maxsize=None)
def _bstems_checker():
    """tests/bstems_check.cpp, built once per process into a directory that goes with the process"""
    import atexit
    import shutil
    import tempfile
    from bstems_util import build_checker
    tmp = tempfile.mkdtemp(prefix="bstems_check_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    return build_checker(tmp)


def _loop(cell, sigma=None, schedule=None):
    c = CELLS[cell]
    gaps = []
    sh = shape(c["graph"])
    rx = samples(cell, sigma)
    ref = ir.loop(decode_callable(cell, schedule, gaps), graph(c["graph"])[3], sh, rx, c["sigma"] if sigma is None else sigma,
                  ir.MAXLOG, PASSES, ir.MAXLOG)
    for x in ref:
        x.setflags(write=False)
    return ref, (min(gaps) if gaps else None)


ORACLE_KW = ("ems_nm", "ems_nc", "tems_nr", "tems_nc")
_REFS = {}


def _shared(cell, schedule=None):
    """cells that differ only in the kernel a debug switch selects (variants 1 and 2 of a fused family) share one reference"""
    c = CELLS[cell]
    key = (c["graph"], c["family"], schedule or c["schedule"], c["max_iter"], c["sigma"], c["B"],
           tuple(sorted((k, v) for k, v in c["kw"].items() if k in ORACLE_KW)))
    if key not in _REFS:
        _REFS[key] = _loop(cell, schedule=schedule)
    return _REFS[key]


def reference(cell):
    """((out, converged, iters, passes_used) of the reference loop, smallest decide gap or None); computed once.  For ems_osd: the
    oracle's EMS loop, whose out_sym differs on the frames OSD rewrites."""
    return _shared(cell)


def flooding_reference(cell):
    """the reference loop of a layered cell's frames under the flooding schedule"""
    return _shared(cell, "flooding")[0]


def counts(conv, used):
    """(converged in pass 1, in a later pass, never)"""
    conv, used = np.asarray(conv), np.asarray(used)
    return int(((conv == 1) & (used == 1)).sum()), int(((conv == 1) & (used > 1)).sum()), int((conv == 0).sum())


def hard_condition(cnt):
    """a frame converges in pass 1; two or more go into pass 2"""
    return cnt[0] >= 1 and cnt[1] + cnt[2] >= 2


def full_mix(cnt):
    return cnt[0] >= 1 and cnt[1] >= 1 and cnt[2] >= 2


def first_pass_llr(cell):
    c = CELLS[cell]
    sh = shape(c["graph"])
    return dg.demod(sh["points"], sh["src"], samples(cell), c["sigma"], sh["N"], sh["p"], dg.MAXLOG)[0]


def scan(cell, sigmas):
    """[(sigma, counts, smallest gap)] of a cell's reference loop at each sigma: how the sigma of CELLS was chosen"""
    rows = []
    for s in sigmas:
        ref, gap = _loop(cell, float(s))
        rows.append((float(s), counts(ref[1], ref[3]), gap))
    return rows


if __name__ == "__main__":
    import os
    import time
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")):
        sys.path.insert(0, p)
    t0 = time.time()
    for s, cnt, gap in scan(sys.argv[1], [float(x) for x in sys.argv[2:]]):
        print(f"{sys.argv[1]} sigma {s:g}: pass 1 / later / never = {cnt}" + (f", smallest gap {gap:.3e}" if gap is not None else ""), flush=True)
    print(f"{time.time() - t0:.1f} s")
