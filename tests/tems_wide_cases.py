"""The cases of T-EMS decoding on codes whose trellis path does not fit nbl_create's 32-bit code (nbl_create_tems_wide, check degrees up
to NBL_TEMS_MAX_CHECK_DEGREE = 32 over any field) -- TEST INFRASTRUCTURE ONLY.  tests/test_tems_wide.py puts on them, without a GPU, the
conditions every GPU case must meet; tests/test_gpu_tems_wide.py compares the kernels of nbl_cn_tems_wide.hip with the references made
here (each computed once per process, shared and read-only).  The reference is the canonical oracle (oracle/nbl_oracle.c, whose T-EMS
arrays are sized by the check degree and which is pinned to the compiled reference at these degrees by the deg_wide_*_tems fixtures):
its decoder under the flooding schedule, its single-check entry point inside tests/layered_tems_ref.py under the damped layered one.

Frames: ems_wide_cases.bpsk_frames -- all-zero-codeword BPSK / AWGN LLRs at the graph's own rate, one frame per Eb/N0 level; real-valued,
so free of ties (asserted: every decision has a positive margin).  Under both schedules one frame converges at iteration 1, one later
and one never within MAX_ITER."""
import functools

import numpy as np

import nbldpc_amd as nb
import layered_ref as lr
import layered_tems_ref as ltr
import pyoracle
from degree_util import degree_code
from ems_wide_cases import bpsk_frames, margin  # noqa: F401  (margin: re-exported for the tests)
from fht_wide_cases import MIX_DEGS, WIDE_DEGS
from test_layered import oracle_edges

MAX_ITER = 4
GRAPH_SEED, FRAME_SEED = 91, 5
LEVELS = (3.0, 5.0, 6.0, 8.0, 1.0, 11.0)
SCHEDULES = ("flooding", "greedy")
B_BATCH = 9

# name -> (q, (check degrees, variable degrees, M), T-EMS parameters)
CASES = {
    "gf64-nc2": (64, WIDE_DEGS, dict(tems_nr=2, tems_nc=2)),
    "gf64-nc3": (64, WIDE_DEGS, dict(tems_nr=2, tems_nc=3)),
    "gf16-shaped": (16, WIDE_DEGS, dict(tems_nr=3, tems_nc=3, tems_factor=1.1, tems_offset=0.1)),
    "gf4-nr1": (4, WIDE_DEGS, dict(tems_nr=1, tems_nc=4)),
    "gf64-dc6-8": (64, ([6, 7, 8], [2, 3], 8), dict(tems_nr=2, tems_nc=3)),          # maxdc <= 8: only the 48-bit path makes it a wide code
    "gf256-dc5-9": (256, ([5, 6, 8, 9], [2, 3], 8), dict(tems_nr=2, tems_nc=2)),
    "gf256-dc17": (256, ([9, 12, 16, 17], [2, 3], 8), dict(tems_nr=2, tems_nc=2)),
    "gf256-dc32": (256, ([9, 16, 32], [2, 3], 6), dict(tems_nr=2, tems_nc=2)),
    "gf128-mix": (128, MIX_DEGS, dict(tems_nr=3, tems_nc=2)),
    "gf16-nc4": (16, ([9, 10], [2, 3], 12), dict(tems_nr=2, tems_nc=4)),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """(code, T-EMS parameters, L [F][N][q-1]) of a named case; built once, L read-only"""
    q, (chk, var, M), kw = CASES[name]
    code = degree_code(q, GRAPH_SEED, chk, var, M)[0]
    L = bpsk_frames(np.random.default_rng(FRAME_SEED), code, LEVELS)
    L.setflags(write=False)
    return code, kw, L


def batch(name, B=B_BATCH):
    """the frames of a case repeated up to B codewords: frame b of the batch is frame b % F of the case"""
    L = wide_case(name)[2]
    return np.ascontiguousarray(L[np.arange(B) % L.shape[0]])


def layer_of(name, which):
    return None if which == "flooding" else nb.layer_greedy(wide_case(name)[0])


@functools.lru_cache(maxsize=None)
def oracle_decoder(code_key, iters, fixed, kw_items):
    """the canonical T-EMS oracle on a code (code_key: a case name, or an nb.Code kept alive by the caller)"""
    code = wide_case(code_key)[0] if isinstance(code_key, str) else code_key
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    return pyoracle.Decoder(ocode, gf, pyoracle.TEMS, iters, pyoracle.CANONICAL, fixed_iters=fixed, **dict(kw_items)), gf


def reference(code_key, kw, L, which, fixed=0, iters=MAX_ITER):
    """[(out, converged, iters, post, c2v, v2c)] per frame of L under schedule `which` (flooding | greedy) from the canonical oracle;
    post [N][q-1], c2v and v2c [E][q-1] in variable-major edge order, as nbl_read_state returns them"""
    od, gf = oracle_decoder(code_key, iters, fixed, tuple(sorted(kw.items())))
    code = wide_case(code_key)[0] if isinstance(code_key, str) else code_key
    ref = []
    for b in range(L.shape[0]):
        if which == "flooding":
            r, out, it = od.decode(L[b])
            post, v2c, c2v = od.state()
            ref.append((out.copy(), int(r), int(it), post, c2v, v2c))
        else:
            ref.append(ltr.decode(od, gf.mul, L[b], nb.layer_greedy(code), iters, fixed_iters=fixed)[:6])
    for r in ref:
        for x in (r[0], r[3], r[4], r[5]):
            x.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def wide_reference(name, which, fixed=0, iters=MAX_ITER):
    code, kw, L = wide_case(name)
    return reference(name, kw, L, which, fixed, iters)


TIES_CASE = "gf64-nc3"


@functools.lru_cache(maxsize=None)
def ties_frames(F=2):
    """[F][N][q-1] integer-valued LLRs in -3 .. 1 on the graph of TIES_CASE: every sum of the check node is exact and many path costs are
    equal, so that the rule for equal costs -- the first path in enumeration order -- decides outputs (tests/test_tems_wide.py shows that it
    does: the opposite rule gives other c2v on these frames)"""
    code = wide_case(TIES_CASE)[0]
    L = np.random.default_rng(FRAME_SEED + 1).integers(-3, 2, (F, code.N, code.q - 1)).astype(np.float64)
    L.setflags(write=False)
    return L
