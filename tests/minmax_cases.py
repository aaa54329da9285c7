"""The cases of Min-Max decoding (method 3, nbl_create_minmax) -- TEST INFRASTRUCTURE ONLY.  tests/test_minmax.py puts on them, without a
GPU, the conditions every GPU case must meet; tests/test_gpu_minmax.py compares the kernels of nbl_cn_minmax.hip with the references made
here (each computed once per process, shared and read-only).  The reference is tests/minmax_ref.py, the header's definition in numpy.

Built like tests/ems_wide_cases.py: degree_code(q, 91, ...), all-zero-codeword BPSK / AWGN frames from default_rng(5) at the graph's own
rate, one frame per Eb/N0 level, MAX_ITER 4, frames repeated up to B = 9.  These are the smallest graphs on which every structural
branch of the programme runs: lanes beyond q idle (mix4, wide16, shaped16), one / two / four waves per check (wide64, mix128, wide256 and
ring256-dc4), an edge count the wave count does not divide (degrees 9, 17, 31 at two and four waves), degree 2 without a step, the first,
the last and a middle output, degree 32, the largest LDS block (wide256), shaping (shaped16), and the shipped codes' shape (ring256-dc4)."""
import functools

import numpy as np

import nbldpc_amd as nb
import minmax_ref as mr
from degree_util import degree_code, ring_code
from ems_wide_cases import bpsk_frames
from fht_wide_cases import MIX_DEGS, WIDE_DEGS

MAX_ITER = 4
GRAPH_SEED, FRAME_SEED = 91, 5
LEVELS = (1.0, 3.0, 5.0, 6.0, 8.0, 11.0)
SCHEDULES = ("flooding", "greedy")
B_BATCH = 9

# name -> (q, (check degrees, variable degrees, M) or a ring's (M, dc), shaping, Eb/N0 levels in dB)
CASES = {
    "wide16": (16, WIDE_DEGS, {}, LEVELS),
    "wide64": (64, WIDE_DEGS, {}, LEVELS),
    "mix4": (4, MIX_DEGS, {}, LEVELS),
    "mix128": (128, MIX_DEGS, {}, LEVELS),
    "wide256": (256, ([9, 16, 32], [2, 3], 6), {}, LEVELS),
    "shaped16": (16, ([9, 10], [2, 3], 12), dict(ems_factor=1.1, ems_offset=0.1), LEVELS),
    "ring256-dc4": (256, (8, 4), {}, LEVELS),
}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, shaping parameters, L [F][N][q-1]) of a named case; built once, L read-only"""
    q, degs, kw, levels = CASES[name]
    code = ring_code(q, *degs) if len(degs) == 2 else degree_code(q, GRAPH_SEED, *degs)[0]
    L = bpsk_frames(np.random.default_rng(FRAME_SEED), code, levels)
    L.setflags(write=False)
    return code, kw, L


def batch(name, B=B_BATCH):
    """the frames of a case repeated up to B codewords: frame b of the batch is frame b % F of the case"""
    L = case(name)[2]
    return np.ascontiguousarray(L[np.arange(B) % L.shape[0]])


def layer_of(name, which):
    """None (flooding), the library's greedy assignment, or one check per layer (serial)"""
    code = case(name)[0]
    return None if which == "flooding" else np.arange(code.M, dtype=np.int32) if which == "serial" else nb.layer_greedy(code)


@functools.lru_cache(maxsize=None)
def checker(name):
    code, kw, _ = case(name)
    return mr.MinMax(code, np.array(nb.datafiles.gf_tables(code.q)[0]), kw.get("ems_factor", 1.0), kw.get("ems_offset", 0.0))


@functools.lru_cache(maxsize=None)
def reference(name, which, fixed=0, iters=MAX_ITER):
    """[(out, converged, iters, post, c2v)] per frame of a case under schedule `which` (flooding | greedy | serial); post [N][q-1], c2v
    [E][q-1] in variable-major edge order, as nbl_read_state returns them"""
    L = case(name)[2]
    ref = [mr.decode(checker(name), L[b], layer_of(name, which), iters, fixed) for b in range(L.shape[0])]
    for r in ref:
        for x in (r[0], r[3], r[4]):
            x.setflags(write=False)
    return ref


def spread(ref):
    """(frames that never converge, that converge after iteration 1, that converge at iteration 1)"""
    never = sum(1 for r in ref if not r[1])
    later = sum(1 for r in ref if r[1] and r[2] > 1)
    first = sum(1 for r in ref if r[1] and r[2] == 1)
    return never, later, first
