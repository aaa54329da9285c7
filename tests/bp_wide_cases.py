"""The cases of exact log-QSPA decoding on codes with checks above degree 8 (nbl_create_bp_wide, check degrees up to
NBL_BP_MAX_CHECK_DEGREE = 32) -- TEST INFRASTRUCTURE ONLY.  tests/test_bp_wide.py puts on them, without a GPU, the margin condition every
GPU case must meet; tests/test_gpu_bp_wide.py compares the kernels of nbl_cn_bp_wide.hip with the references made here (each computed
once per process, shared and read-only).  The reference is the FP64 restatement: the oracle's log-QSPA single-check entry point inside
tests/bp_wide_ref.py (flooding) and tests/layered_bp_ref.py (layered, as it is).

Frames: _frames of tests/test_layered_bp.py -- n = normal(-2, 4), w = normal(-900, 700) (the mantissa / exponent path of the
convolutions), m = narrow and wide vectors mixed in one check.  Seeds are chosen on the CPU with the restatement alone until every
decision of the schedule has a gap of at least GAP_MIN (tests/test_bp_wide.py asserts it): a condition on the inputs, not on any kernel.
The oracle needs about 5 s per frame and iteration on the GF(256) graph, hence its two frames and two iterations."""
import concurrent.futures
import functools

import numpy as np

import nbldpc_amd as nb
import bp_wide_ref
import layered_bp_ref as lbr
import layered_ref as lr
import pyoracle
from degree_util import degree_code
from fht_wide_cases import MIX_DEGS, WIDE_DEGS
from test_abi import _ring_code
from test_layered import oracle_edges
from test_layered_bp import GAP_MIN, _bpsk_llr_zero, _frames  # noqa: F401  (GAP_MIN: re-exported for the tests)

# name -> (q, graph seed, (check degrees, variable degrees, M), frame kinds, iterations)
SYNTHETIC = {
    "gf64": (64, 92, ([9, 17, 32], [2, 3], 6), "nwm", 3),        # one wave; narrow and wide vectors in one check
    "gf256": (256, 91, ([9, 16, 32], [2, 3], 6), "nw", 2),       # four waves, 76,032 B of LDS: the launcher opts in
    "gf128-mix": (128, 95, MIX_DEGS, "n", 3),                    # two waves; degree 2, the 8 / 9 boundary, variables of degree 1 and 8
    "gf16": (16, 93, WIDE_DEGS, "n", 3),                         # mostly idle lanes
    "gf4": (4, 94, WIDE_DEGS, "n", 3),
}
RING = "ring16-dc16"                                             # _ring_code(16, 12, 16): N = 96, rate 7/8; 6 frames at 6 dB, 8 iterations
NAMES = tuple(SYNTHETIC) + (RING,)
SCHEDULES = ("flooding", "greedy")
B_BATCH = 9


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """(code, L [F][N][q-1], max_iter) of a named case; built once, L read-only"""
    if name == RING:
        code = _ring_code(16, 12, 16)
        L, iters = _bpsk_llr_zero(np.random.default_rng(77), code, 6, 6.0), 8
    else:
        q, seed, (chk, var, M), kinds, iters = SYNTHETIC[name]
        code = degree_code(q, seed, chk, var, M)[0]
        L = _frames(np.random.default_rng(seed), code.N, q, kinds)
    L.setflags(write=False)
    return code, L, iters


def layer_of(name, which):
    return None if which == "flooding" else nb.layer_greedy(wide_case(name)[0])


def batch(name, B=B_BATCH):
    """the frames of a case repeated up to B codewords: frame b of the batch is frame b % F of the case"""
    L = wide_case(name)[1]
    return np.ascontiguousarray(L[np.arange(B) % L.shape[0]])


@functools.lru_cache(maxsize=None)
def oracle_code(name):
    code = wide_case(name)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    return ocode, gf


@functools.lru_cache(maxsize=None)
def wide_reference(name, which, fixed=0):
    """[(out, converged, iters, post, c2v, v2c, gap)] per frame of a case under schedule `which` (flooding | greedy) from the FP64
    restatement; post [N][q-1], c2v and v2c [E][q-1] in variable-major edge order.  The time goes into the oracle's check-node update,
    which leaves the interpreter lock alone: one oracle decoder and one thread per frame."""
    code, L, iters = wide_case(name)
    ocode, gf = oracle_code(name)
    lay = layer_of(name, which)

    def one(b):
        od = pyoracle.Decoder(ocode, gf, pyoracle.BP, iters, pyoracle.CANONICAL, fixed_iters=fixed)
        if lay is None:
            r = bp_wide_ref.decode_flooding(od, gf.mul, L[b], iters, fixed)
        else:
            r = lbr.decode(od, gf.mul, L[b], lay, iters, fixed_iters=fixed)
            r = r[:6] + (r[8],)
        for x in (r[0], r[3], r[4], r[5]):
            x.setflags(write=False)
        return r

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(L.shape[0], 8)) as pool:
        return list(pool.map(one, range(L.shape[0])))
