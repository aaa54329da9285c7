"""The cases of EMS decoding on codes with checks above degree 8 (nbl_create_ems_wide, check degrees up to
NBL_EMS_MAX_CHECK_DEGREE = 32) -- TEST INFRASTRUCTURE ONLY.  tests/test_ems_wide.py puts on them, without a GPU, the conditions every
GPU case must meet; tests/test_gpu_ems_wide.py compares the kernels of nbl_cn_ems_wide.hip with the references made here (each computed
once per process, shared and read-only).  The reference is the canonical oracle (oracle/nbl_oracle.c, generic in the check degree and
pinned to the compiled reference at these degrees by the deg_wide_* fixtures): its decoder under the flooding schedule, its single-check
entry point inside tests/layered_ref.py under the layered one.

Frames: all-zero-codeword BPSK / AWGN LLRs at the graph's own rate 1 - M/N, one frame per Eb/N0 level of the case; real-valued, so free of
ties (asserted: every decision has a positive margin).  The levels of a case are chosen on the oracle alone so that under both schedules
one frame converges at iteration 1, one later and one never within MAX_ITER."""
import functools

import numpy as np

import nbldpc_amd as nb
import layered_ref as lr
import pyoracle
from degree_util import degree_code
from fht_wide_cases import MIX_DEGS, WIDE_DEGS
from test_layered import oracle_edges

MAX_ITER = 4
GRAPH_SEED, FRAME_SEED = 91, 5
LEVELS = (3.0, 5.0, 6.0, 8.0, 1.0)     # 3 / 5 / 6 / 8 dB: never, at iteration 3, at 2 and at 1 in most cases; 1 dB: never, in every case
HIGH = LEVELS + (11.0,)               # the (9, 10) graph converges at iteration 2 at 8 dB: one frame that converges at once
SCHEDULES = ("flooding", "greedy")
B_BATCH = 9

# name -> (q, (check degrees, variable degrees, M), EMS parameters, Eb/N0 levels in dB)
CASES = {
    "gf64-nm8": (64, WIDE_DEGS, dict(ems_nm=8, ems_nc=2), LEVELS),
    "gf64-nm16": (64, WIDE_DEGS, dict(ems_nm=16, ems_nc=3), LEVELS),
    "gf16-shaped": (16, WIDE_DEGS, dict(ems_nm=6, ems_nc=2, ems_factor=1.1, ems_offset=0.1), LEVELS),
    "gf4-full": (4, WIDE_DEGS, dict(ems_nm=4, ems_nc=3), LEVELS),
    "gf256-dc17": (256, ([9, 12, 16, 17], [2, 3], 8), dict(ems_nm=8, ems_nc=2), LEVELS),
    "gf256-nm12": (256, ([9, 16, 32], [2, 3], 6), dict(ems_nm=12, ems_nc=3), LEVELS),
    "gf128-mix": (128, MIX_DEGS, dict(ems_nm=8, ems_nc=3), LEVELS),
    "gf16-nc9": (16, ([9, 10], [2, 3], 12), dict(ems_nm=4, ems_nc=9), HIGH),
    "gf16-nc0": (16, ([9, 10], [2, 3], 12), dict(ems_nm=4, ems_nc=0), HIGH),
}
NAMES = tuple(CASES)


def bpsk_frames(rng, code, levels):
    """[len(levels)][N][q-1]: symbol LLRs of the all-zero codeword over BPSK / AWGN at rate 1 - M/N, one frame per level"""
    p = code.q.bit_length() - 1
    a = np.arange(1, code.q)
    mask = ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64)
    rate = 1.0 - code.M / code.N
    L = []
    for ebn0 in levels:
        sigma = 1.0 / np.sqrt(2 * rate * 10 ** (ebn0 / 10.0))
        bit = -2.0 * (1.0 + sigma * rng.standard_normal((code.N, p))) / sigma ** 2
        L.append(bit @ mask.T)
    return np.array(L)


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """(code, EMS parameters, L [F][N][q-1]) of a named case; built once, L read-only"""
    q, (chk, var, M), kw, levels = CASES[name]
    code = degree_code(q, GRAPH_SEED, chk, var, M)[0]
    L = bpsk_frames(np.random.default_rng(FRAME_SEED), code, levels)
    L.setflags(write=False)
    return code, kw, L


def batch(name, B=B_BATCH):
    """the frames of a case repeated up to B codewords: frame b of the batch is frame b % F of the case"""
    L = wide_case(name)[2]
    return np.ascontiguousarray(L[np.arange(B) % L.shape[0]])


def layer_of(name, which):
    return None if which == "flooding" else nb.layer_greedy(wide_case(name)[0])


@functools.lru_cache(maxsize=None)
def _oracle(name, iters, fixed):
    code, kw, _ = wide_case(name)
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    return pyoracle.Decoder(ocode, gf, pyoracle.EMS, iters, pyoracle.CANONICAL, fixed_iters=fixed, **kw), gf


@functools.lru_cache(maxsize=None)
def wide_reference(name, which, fixed=0, iters=MAX_ITER):
    """[(out, converged, iters, post, c2v)] per frame of a case under schedule `which` (flooding | greedy) from the canonical oracle;
    post [N][q-1], c2v [E][q-1] in variable-major edge order, as nbl_read_state returns them"""
    od, gf = _oracle(name, iters, fixed)
    L = wide_case(name)[2]
    ref = []
    for b in range(L.shape[0]):
        if which == "flooding":
            r, out, it = od.decode(L[b])
            post, _, c2v = od.state()
            ref.append((out.copy(), int(r), int(it), post, c2v))
        else:
            ref.append(lr.decode(od, gf.mul, L[b], layer_of(name, which), iters, fixed_iters=fixed))
    for r in ref:
        for x in (r[0], r[3], r[4]):
            x.setflags(write=False)
    return ref


def margin(post):
    """the smallest distance between the largest and the second largest entry of a posterior vector, the implicit 0 of symbol 0
    included: positive = no decision of the frame is a tie"""
    full = np.concatenate([np.zeros((post.shape[0], 1)), post], axis=1)
    top = np.sort(full, axis=1)[:, -2:]
    return float(np.min(top[:, 1] - top[:, 0]))
