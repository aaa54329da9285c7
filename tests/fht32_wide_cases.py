"""The cases of single-precision FHT decoding on codes with checks above degree 8 (nbl_create_fht32_wide, check degrees up to
NBL_FHT32_MAX_CHECK_DEGREE = 32) -- TEST INFRASTRUCTURE ONLY.  tests/test_fht32_wide.py puts on them, without a GPU, the conditions
tests/test_fht32.py::test_conditions_on_every_gpu_case puts on a GPU case, and the noise condition of the 2^-16 floor;
tests/test_gpu_fht32_wide.py compares the kernels of nbl_cn_fht32_wide.hip with the references made here (each computed once per process
and shared).  The restatement is tests/fht32_wide_ref.py.

Codes come from tests/fht_wide_cases.py::wide_case.  Frames: that function's where they meet the float32 conditions under both
schedules; otherwise the first of a seed range (4200 on, chosen on the CPU with the two evaluations of the restatement alone: a
condition on the inputs, not on any kernel) that does -- FRAME_SEEDS, one entry per frame (None keeps the frame), the frame kinds of
the FP64 case.  The frames of the ring case are six of that range that converge at different iterations and never.

flat-256: the wide-256 code; in every frame one third of the variables carry the all-zero channel vector (a punctured symbol): the
first FLAT_IN_32 variables of the first degree-32 check (one of them joins the first degree-9 check), then, one at a time, the
variable of lowest index among those that join the fewest checks which are still without a flat variable or are that degree-9 check.
A flat input transforms to U = (q, 0, .., 0), so 16 of them alone make a product of 2^128: the unscaled float32 update leaves
binary32's range at that check, the scaled one (step 3a) does not.  Two flat inputs make every output of a check exactly zero, which
is why the set is kept together: the degree-9 check keeps exactly one flat variable (whose message is then the only non-zero one) and
the other degree-9 check none, so that the frames carry messages at all.  An exactly-zero vector decides 0 in every implementation
without a rounding being involved, so it has no decision gap to measure: gap_nonzero() leaves such vectors out.

SW3: the cases of tests/test_fht32.py (check degrees up to 8) on which tests/test_gpu_fht32_wide.py compares the register programme
with the wide one (nbl_debug_force_generic(dec, 3)), keyed "sw3:<case>": that file's frames where they meet the conditions under the
scaled update too, frames of the same kind from the seed range otherwise.  Both restatements are made here on the same frames: the
scaled one (reference) and the unscaled one of tests/fht32_ref.py (register_reference), whose recorded deviation is D32R."""
import functools
from unittest import mock

import numpy as np

import nbldpc_amd as nb
import fht_ref as fr
import fht32_ref as f32
import fht32_wide_ref as fw
import fht_wide_cases as wc
import pyoracle
from layered_bp_ref import _gap
from test_fht32 import GAP_FACTOR, NEAR, TOL_CAP, _near_top_difference, fht32_case
from test_layered import oracle_edges
from test_layered_bp import _bpsk_llr_zero, _frames

FLAT = "flat-256"
RING = wc.RING
NAMES = ("wide-256", "wide-64", "wide-128", "wide-16", "wide-4", "mix-256", "mix-16", RING, FLAT)
SCHEDULES = ("flooding", "greedy")
SW3 = ("gf16", "ring256", "ring64", "all-16", "rand128")
NOISE_MAX = 2.0 ** -18       # largest |v32 - v80| / t: a relative error of 1/4 or less at the floor

# name -> per frame a seed or None (the frame of wide_case / fht32_case stays), where those frames do not meet the float32 conditions
FRAME_SEEDS = {
    "wide-64": (None, None, 4200),
    "mix-256": (4200,),
    "mix-16": (5029,),
    RING: (4211, 4212, 4238, 4287, 4310, 4270),
    "sw3:gf16": (None, None, 4209, None, None, None, None, 4212),
    "sw3:all-16": (4650,),
}
# fewer iterations where 3 meet the conditions at no seed tried (sw3:all-16 has 2 from tests/test_fht32.py; sw3:rand128: none of 1400)
ITERS = {"sw3:rand128": 2}
FLAT_SEED = 4200             # the two normal(-2, 4) frames of flat-256
FLAT_IN_32 = 16              # flat variables taken from the first degree-32 check
# where each frame of RING converges under the float32 restatement, both evaluations alike (0 = never within 8 iterations)
RING_ITERS = {"flooding": (2, 3, 0, 0, 3, 0), "greedy": (2, 2, 0, 8, 2, 0)}   # (greedy, frame 3: at the last iteration)
RING_LAYERS = wc.RING_LAYERS
# (sw3 case, schedule) -> the deviation between the two evaluations of the UNSCALED restatement on this file's frames (D32 of fht32_ref)
D32R = {
    ("sw3:gf16", "flooding"): 2.535e-06,
    ("sw3:gf16", "greedy"): 2.309e-06,
    ("sw3:ring256", "flooding"): 7.794e-06,
    ("sw3:ring256", "greedy"): 6.590e-06,
    ("sw3:ring64", "flooding"): 1.338e-06,
    ("sw3:ring64", "greedy"): 3.311e-05,
    ("sw3:all-16", "flooding"): 1.220e-06,
    ("sw3:all-16", "greedy"): 1.028e-05,
    ("sw3:rand128", "flooding"): 3.088e-06,
    ("sw3:rand128", "greedy"): 3.722e-06,
}


def kinds(name):
    """frame kinds of a case: n, w, m as tests/test_layered_bp.py::_frames has them; b = the all-zero codeword over BPSK (6 dB on the
    ring code, 1.5 dB on the shipped GF(16) code); q = normal(-2, 4) / 4.  mix-256 takes q: beside checks of degree 2 .. 4 a
    normal(-2, 4) frame puts many outputs at the floor, where the two evaluations differ by 2^-8 relative (one rounding of exp, 2^-24
    of the largest, against 2^-16), so every decision would need a gap of 64 x 1e-3 or more -- which no such frame of 54 GF(256)
    variables has (none of 1700 tried).  Vectors a quarter as wide keep the outputs above the floor, and the margin is that of the
    other cases.  (Wider vectors have the gaps too, but at magnitudes of 200 one float32 rounding of a sum is 1.5e-5, the size of the
    tolerance: the probability-domain statement is for LLRs whose ulp lies far below it.)"""
    if name == "mix-256":
        return "q"
    if name == RING:
        return "b" * 6
    if name.startswith("sw3:"):
        return "b" * 8 if name == "sw3:gf16" else "nwm" if name.startswith("sw3:ring") else "n"
    return wc.SYNTHETIC[name][3]


def make_frame(name, code, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "q":
        return 0.25 * rng.normal(-2, 4, (code.N, code.q - 1))
    return _bpsk_llr_zero(rng, code, 1, 6.0 if name == RING else 1.5)[0] if kind == "b" else _frames(rng, code.N, code.q, kind)[0]


@functools.lru_cache(maxsize=None)
def flat_set():
    """the variables of flat-256 that carry the all-zero channel vector: a third of them"""
    code = wc.wide_case("wide-256")[0]
    off, voff = np.concatenate([[0], np.cumsum(code.chk_deg)]), np.concatenate([[0], np.cumsum(code.var_deg)])
    m32, m9 = int(np.argmax(code.chk_deg == 32)), int(np.argmax(code.chk_deg == 9))
    flat = code.chk_var[off[m32]:off[m32] + FLAT_IN_32].tolist()
    while len(flat) < code.N // 3:
        have = flat_per_check(code, flat)
        flat.append(min((n for n in range(code.N) if n not in flat),
                        key=lambda n: (sum(have[m] == 0 or m == m9 for m in code.var_chk[voff[n]:voff[n + 1]]), n)))
    return np.sort(np.array(flat))


def flat_per_check(code, flat):
    """how many variables of `flat` each check joins"""
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    return [int(np.isin(code.chk_var[off[m]:off[m + 1]], flat).sum()) for m in range(code.M)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, L, max_iter) of a named case; built once"""
    if name == FLAT:
        code = wc.wide_case("wide-256")[0]
        L = _frames(np.random.default_rng(FLAT_SEED), code.N, code.q, "nn")
        L[:, flat_set(), :] = 0.0
        return code, L, 3
    code, L, iters = fht32_case(name[4:]) if name.startswith("sw3:") else wc.wide_case(name)
    if name in FRAME_SEEDS:
        assert len(FRAME_SEEDS[name]) == L.shape[0] == len(kinds(name))
        L = np.stack([L[b] if seed is None else make_frame(name, code, kind, seed) for b, (kind, seed) in enumerate(zip(kinds(name), FRAME_SEEDS[name]))])
    return code, L, ITERS.get(name, iters)


@functools.lru_cache(maxsize=None)
def checks(name):
    """the scaled float32 check of a case's code under the two evaluations of exp / log"""
    code = case(name)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    return fw.Fht32WideCheck(ocode, gf.mul), fw.Fht32WideCheck(ocode, gf.mul, via64=True)


@functools.lru_cache(maxsize=None)
def register_checks(name):
    """the unscaled float32 check of tests/fht32_ref.py on the same code, under the two evaluations"""
    chk = checks(name)[0]
    return f32.Fht32Check(chk.code, chk.mul), f32.Fht32Check(chk.code, chk.mul, via64=True)


def layer_of(name, which):
    return None if which == "flooding" else nb.layer_greedy(case(name)[0])


def gap_nonzero(P):
    """fht_ref's decision gap, infinite for an exactly-zero vector"""
    return _gap(P) if np.any(P) else np.inf


def decode(chk, L, lay, iters, fixed=0):
    """fht_ref.decode with the decision gap taken over the vectors that are not exactly zero (fht_ref calls _gap by its module-level name)"""
    with mock.patch.object(fr, "_gap", gap_nonzero):
        return fr.decode(chk, L, lay, iters, fixed)


@functools.lru_cache(maxsize=None)
def reference(name, which, fixed=0, via64=False):
    """[(out, converged, iters, post, c2v, v2c, gap)] per frame of a case under schedule `which` (flooding | greedy) in float32 with the
    scaled check (numpy's exp / log, or the second evaluation); computed once and shared"""
    _, L, iters = case(name)
    return [decode(checks(name)[int(via64)], L[b], layer_of(name, which), iters, fixed) for b in range(L.shape[0])]


@functools.lru_cache(maxsize=None)
def register_reference(name, which, via64=False):
    """the same under the unscaled update of tests/fht32_ref.py (the SW3 cases: what the register programme is compared with)"""
    _, L, iters = case(name)
    return [decode(register_checks(name)[int(via64)], L[b], layer_of(name, which), iters) for b in range(L.shape[0])]


def tolerance(name, which, fixed=0):
    """the GPU tolerance of a case: 16 x its recorded D32W"""
    return 16.0 * fw.D32W[(name + "-fixed" if fixed else name, which)]


def frame_figures(a, x):
    """of one frame under the two evaluations: (same decisions, flags and counts; finite float32 state; smallest gap; largest difference
    near a vector's top; deviation in the probability domain)"""
    same = bool(np.array_equal(a[0], x[0]) and (a[1], a[2]) == (x[1], x[2]))
    sound = all(np.all(np.isfinite(a[k])) and a[k].dtype == np.float32 for k in (3, 4, 5))
    return same, sound, min(a[6], x[6]), _near_top_difference(a, x), fr.state_dev(a, x)


def frame_ok(fig):
    """the conditions of tests/test_fht32.py::test_conditions_on_every_gpu_case on one frame"""
    same, sound, gap, diff, d = fig
    return same and sound and gap >= GAP_FACTOR * diff and gap >= 1e-6 and 16.0 * d <= TOL_CAP


def noise(name, which):
    """largest |v32 - v80| / t over every check the case evaluates under schedule `which`, per frame"""
    _, L, iters = case(name)
    chk = checks(name)[0]
    worst = []

    class Probe(fw.Fht32WideCheck):
        def check(self, m, vin):
            g = self.g
            worst[-1] = max(worst[-1], fw.noise_over_t(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul))
            return super().check(m, vin)

    probe = Probe(chk.code, chk.mul)
    for b in range(L.shape[0]):
        worst.append(0.0)
        decode(probe, L[b], layer_of(name, which), iters)
    return worst


assert NEAR == 16.0          # (what _near_top_difference calls "near the top")
