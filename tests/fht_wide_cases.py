"""The cases of FHT sum-product decoding on codes with checks above degree 8 (nbl_create_fht, check degrees up to
NBL_FHT_MAX_CHECK_DEGREE = 32) -- TEST INFRASTRUCTURE ONLY.  tests/test_fht_wide.py puts on them, without a GPU, the conditions
tests/test_fht.py::test_conditions_on_every_gpu_case puts on a GPU case; tests/test_gpu_fht_wide.py compares the kernels of
nbl_cn_fht_wide.hip with the references made here (each computed once per process and shared).  The restatement is tests/fht_ref.py
unchanged: it is generic in the check degree.

D80: per (case, schedule) the largest |w(x_fp64) - w(x_80bit)| over post, c2v and v2c of every frame, recorded from
tests/test_fht_wide.py::test_conditions_on_every_wide_case (which recomputes and compares it).  The GPU tolerance is 16 x this figure
(tests/test_gpu_fht.py says why 16)."""
import functools

import numpy as np

import nbldpc_amd as nb
import pyoracle
from degree_util import degree_code
from fht_ref import FhtCheck, check_node, decode, w_dev  # noqa: F401  (check_node, w_dev: for the tests that import this module)
from test_abi import _ring_code
from test_layered import oracle_edges
from test_layered_bp import _bpsk_llr_zero, _frames

WIDE_DEGS = ([9, 12, 16, 17, 24, 32], [2, 3], 12)                # check degrees, variable degrees, M: N = 88
MIX_DEGS = ([2, 3, 4, 8, 9, 10, 31, 32], [1, 2, 3, 8], 16)       # N = 54: degree 2, the edge degrees 8 / 9, variables of degree 1 and 8

# name -> (q, seed, degrees, frame kinds); 3 iterations each
SYNTHETIC = {
    "wide-256": (256, 91, WIDE_DEGS, "nwm"),
    "wide-64": (64, 92, WIDE_DEGS, "nwm"),
    "wide-128": (128, 95, WIDE_DEGS, "nwm"),
    "wide-32": (32, 96, WIDE_DEGS, "n"),
    "wide-16": (16, 93, WIDE_DEGS, "n"),
    "wide-8": (8, 97, WIDE_DEGS, "n"),
    "wide-4": (4, 94, WIDE_DEGS, "n"),
    "mix-256": (256, 99, MIX_DEGS, "n"),
    "mix-16": (16, 98, MIX_DEGS, "n"),
}
RING = "ring16-dc16"                                             # _ring_code(16, 12, 16): N = 96, rate 7/8; 6 frames at 6 dB, 8 iterations
NAMES = tuple(SYNTHETIC) + (RING,)
SCHEDULES = ("flooding", "greedy")
# where each frame of RING converges (0 = never within 8 iterations), from the restatement in FP64 and in 80-bit arithmetic alike
RING_ITERS = {"flooding": (6, 0, 2, 0, 3, 5), "greedy": (5, 0, 2, 0, 2, 3)}
RING_LAYERS = 12

# (case, schedule) -> D80; "-fixed" = fixed_iters = 1
D80 = {
    ("wide-256", "flooding"): 4.776e-11,
    ("wide-256", "greedy"): 4.776e-11,
    ("wide-64", "flooding"): 5.985e-11,
    ("wide-64", "greedy"): 5.985e-11,
    ("wide-128", "flooding"): 3.674e-15,
    ("wide-128", "greedy"): 3.893e-15,
    ("wide-32", "flooding"): 3.884e-15,
    ("wide-32", "greedy"): 3.395e-15,
    ("wide-16", "flooding"): 1.977e-15,
    ("wide-16", "greedy"): 2.062e-15,
    ("wide-8", "flooding"): 1.815e-15,
    ("wide-8", "greedy"): 1.860e-15,
    ("wide-4", "flooding"): 1.651e-15,
    ("wide-4", "greedy"): 1.705e-15,
    ("mix-256", "flooding"): 4.362e-12,
    ("mix-256", "greedy"): 2.235e-12,
    ("mix-16", "flooding"): 7.244e-12,
    ("mix-16", "greedy"): 3.838e-12,
    ("ring16-dc16", "flooding"): 3.271e-14,
    ("ring16-dc16", "greedy"): 1.832e-14,
    ("ring16-dc16-fixed", "flooding"): 3.790e-14,
    ("ring16-dc16-fixed", "greedy"): 1.832e-14,
}


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """(code, L, max_iter) of a named case; built once"""
    if name == RING:
        code = _ring_code(16, 12, 16)
        return code, _bpsk_llr_zero(np.random.default_rng(77), code, 6, 6.0), 8
    q, seed, (chk, var, M), kinds = SYNTHETIC[name]
    code = degree_code(q, seed, chk, var, M)[0]
    return code, _frames(np.random.default_rng(seed), code.N, q, kinds), 3


@functools.lru_cache(maxsize=None)
def _checks(name):
    code = wide_case(name)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    return FhtCheck(ocode, gf.mul), FhtCheck(ocode, gf.mul, np.longdouble)


def layer_of(name, which):
    return None if which == "flooding" else nb.layer_greedy(wide_case(name)[0])


def _reference(name, which, fixed, k):
    _, L, iters = wide_case(name)
    return [decode(_checks(name)[k], L[b], layer_of(name, which), iters, fixed) for b in range(L.shape[0])]


@functools.lru_cache(maxsize=None)
def wide_reference(name, which, fixed=0):
    """[(out, converged, iters, post, c2v, v2c, gap)] per frame of a case under schedule `which` (flooding | greedy) in FP64"""
    return _reference(name, which, fixed, 0)


@functools.lru_cache(maxsize=None)
def wide_reference80(name, which, fixed=0):
    return _reference(name, which, fixed, 1)


def tolerance(name, which, fixed=0):
    """the GPU tolerance of a case: 16 x its recorded D80"""
    return 16.0 * D80[(name + "-fixed" if fixed else name, which)]
