"""Single-precision FHT decoding on codes with checks above degree 8 (nbl_create_fht32_wide, check degrees 2 .. 32) without a GPU: the
export, the plan, the refusals of the entry point, the scaled float32 definition (tests/fht32_wide_ref.py, step 3a) against an 80-bit
brute-force XOR convolution at degrees 9, 16 and 32 and against the unscaled definition at degrees up to 8, the range on flat inputs,
and the conditions on the inputs of every case tests/test_gpu_fht32_wide.py compares with (tests/fht32_wide_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import fht_ref as fr
import fht32_ref as f32
import fht32_wide_cases as cs
import fht32_wide_ref as fw
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_fht import _layer_of
from test_fht32 import CASES, LN_FLOOR, SCHEDULES, TOL_CAP, _create_fht32, _device_stage, _rel, degree9_code, fht32_case, fht32_reference, tolerance
from test_fht32 import _checks as fht32_checks
from test_fht_wide import _graphs
from test_layered import GF16, _refused

BP = dict(method=nb.METHOD_BP, max_iter=5)


def _create_fht32_wide(code, layer_of, flags, params=None):
    """nbl_create_fht32_wide itself at device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in nb.datafiles.gf_tables(code.q))
    prm = params if params is not None else nb.binding.Params(nb.METHOD_BP, 5, 32, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_fht32_wide(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def test_library_exports_nbl_create_fht32_wide():
    # (not in nb.EXPORTS: tests/test_abi.py holds that list equal to the names its pattern finds in the header, and the pattern stops at a digit)
    assert hasattr(nb.load_library(), "nbl_create_fht32_wide")
    assert nb.FHT32_WIDE_LAYERED == 1 and nb.load_library().nbl_abi_version() == 1
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbldpc.h")).read()
    assert "#define NBL_FHT32_MAX_CHECK_DEGREE 32" in text and "#define NBL_FHT32_WIDE_LAYERED 1u" in text


def test_plan_names_the_fht32_wide_kernels():
    """A code with a check above degree 8 -> fht32_wide / fht32_wide_layered under every debug switch; on any other code the plan of
    nbl_create_fht32, except that switch 3 selects the wide programme; never fused, v2c kept.  nbl_create_fht32's own plan does not move."""
    wide, wide_l = ("fht32_wide", False, False, True), ("fht32_wide_layered", False, False, True)
    reg, reg_l = ("fht32", False, False, True), ("fht32_layered", False, False, True)
    for code in [cs.case(name)[0] for name in cs.NAMES] + [_ring_code(16, 20, 32), degree9_code()]:
        assert code.chk_deg.max() > 8
        for fg, rs in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
            assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, force_generic=fg, record_state=rs) == wide
            assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, layers="greedy", force_generic=fg, record_state=rs) == wide_l
    small = [profile_code("all", q)[0] for q in (4, 8, 16, 32, 64, 128, 256)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(256, 12, 8)]
    for code in small:
        assert code.chk_deg.max() <= 8
        for rs in (False, True):
            assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, force_generic=3, record_state=rs) == wide
            assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, layers="greedy", force_generic=3, record_state=rs) == wide_l
            for fg in (0, 1, 2):
                assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, force_generic=fg, record_state=rs) == reg
                assert debug_plan(code, nb.METHOD_BP, fht32_wide=True, layers="greedy", force_generic=fg, record_state=rs) == reg_l
            for fg in (0, 1, 2, 3):                      # "no debug switch moves it"
                assert debug_plan(code, nb.METHOD_BP, fht32=True, force_generic=fg, record_state=rs) == reg
                assert debug_plan(code, nb.METHOD_BP, fht32=True, layers="greedy", force_generic=fg, record_state=rs) == reg_l
    with pytest.raises(ValueError):
        debug_plan(small[0], nb.METHOD_BP, fht32=True, fht32_wide=True)


def test_create_fht32_wide_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    dc32, dc33, dc9, dv9, both = _graphs()
    # ---- the flags, with create_kind's texts ----
    for flags in (2, 3, 1 << 31):
        rc, msg = _create_fht32_wide(code, None, flags)
        assert rc == -1 and "nbl_create_fht32_wide" in msg and "unknown flag bit" in msg and "NBL_FHT32_WIDE_LAYERED" in msg, (flags, rc, msg)
    rc, msg = _create_fht32_wide(code, greedy, 0)
    assert rc == -1 and "nbl_create_fht32_wide" in msg and "layer assignment belongs to the layered schedule" in msg, (rc, msg)
    # ---- valid requests reach the device stage (device -1: they fail there, last): degrees 8, 9 and 32, both schedules ----
    for c in (code, dc9, dc32, cs.case("wide-256")[0]):
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(c), 1)):
            assert _device_stage(*_create_fht32_wide(c, lay, flags)), (c.chk_deg.max(), lay is None, flags)
        for layers in (None, "greedy"):
            kw = dict(layers=layers, fht32_wide=True, **BP)
            if _no_device():
                _refused(c, -3, "no CPU decode path", **kw)
            else:
                nb.Decoder(c, **kw).close()
    # ---- a check of degree 33: NBL_ERR_ARG; the message names the entry point, 33 and 32.  Variable degrees stay 1 .. 8 ----
    for lay, flags in ((None, 0), (None, 1)):
        rc, msg = _create_fht32_wide(dc33, lay, flags)
        assert rc == -1 and "nbl_create_fht32_wide" in msg and "check degree 33 " in msg and "(32)" in msg and "(8)" not in msg, (rc, msg)
    for layers in (None, "greedy"):
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, fht32_wide=True, **BP)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, fht32_wide=True, **BP)
    # ---- nbl_create_fht32 keeps its limit of 8 and its text ----
    nine = degree9_code()
    for c in (nine, dc9):
        for lay, flags in ((None, 0), (None, 1)):
            rc, msg = _create_fht32(c, lay, flags)
            assert rc == -1 and "nbl_create_fht32:" in msg and "check degree 9 " in msg and "(8)" in msg and "nbl_create_fht " in msg, (rc, msg)
        assert _device_stage(*_create_fht32_wide(c, None, 0))
    # ---- any method but 1: NBL_ERR_UNSUPPORTED, the message names method 1 ----
    for method in (nb.METHOD_EMS, nb.METHOD_TEMS, nb.METHOD_OSD, nb.METHOD_BS_TEMS, 3, 0):
        prm = nb.binding.Params(method, 5, 32, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
        for c in (code, dc32):
            for lay, flags in ((None, 0), (None, 1)):
                rc, msg = _create_fht32_wide(c, lay, flags, prm)
                assert rc == -2 and "nbl_create_fht32_wide" in msg and "log-QSPA (method 1) only" in msg, (method, rc, msg)
        _refused(code, -2, "nbl_create_fht32_wide", "log-QSPA (method 1) only", fht32_wide=True, method=method, max_iter=5)
    # ---- every assignment error of nbl_create_layered, with its status and text ----
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    v = int(code.chk_var[0])
    other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
    shared = greedy.copy()
    shared[other] = shared[0]
    bad_neg = greedy.copy()
    bad_neg[3] = -1
    bad_gap = greedy.copy()
    bad_gap[bad_gap == bad_gap.max()] += 1
    bad_big = greedy.copy()
    bad_big[5] = 1 << 30
    _refused(code, -1, "share variable", layers=shared, fht32_wide=True, **BP)
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad_neg, fht32_wide=True, **BP)
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad_gap, fht32_wide=True, **BP)
    _refused(code, -1, "empty layer", layers=bad_big, fht32_wide=True, **BP)
    for lay in (shared, bad_neg, bad_gap, bad_big):      # the same status and text as nbl_create_layered_bp gives
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(code, layers=lay, fht32_wide=True, **BP)
        with pytest.raises(nb.NblError) as f:
            nb.Decoder(code, layers=lay, bp=True, **BP)
        assert (e.value.status, str(e.value)) == (f.value.status, str(f.value))
    # ---- everything else nbl_create refuses, the same way, under both schedules ----
    mul, inv = (np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(16))
    bad_mul = mul.copy()
    bad_mul[3, 5] ^= 1
    zero_h = nb.Code(GF16)
    zero_h.chk_h = zero_h.chk_h.copy()
    zero_h.chk_h[2] = 0
    for layers in (None, "greedy"):
        for c, kw in ((code, dict(method=nb.METHOD_BP, max_iter=-1)), (zero_h, BP), (code, dict(gf=(bad_mul, inv), **BP)),
                      (_ring_code(512, 8, 4), dict(gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **BP))):
            with pytest.raises(nb.NblError) as e:
                nb.Decoder(c, layers=layers, fht32_wide=True, **kw)
            with pytest.raises(nb.NblError) as f:
                nb.Decoder(c, **kw)
            assert f.value.status in (-1, -2) and (e.value.status, str(e.value)) == (f.value.status, str(f.value)), (layers, kw)
    # ---- the Python layer: fht32_wide goes with layers alone ----
    for kw in (dict(fht32=True), dict(fht=True), dict(bp=True, layers="greedy"), dict(damped=True, layers="greedy"), dict(bp_wide=True), dict(osd_order=0),
               dict(bs_nm=4), dict(wide=True), dict(tems_wide=True)):
        with pytest.raises(ValueError):
            nb.Decoder(code, fht32_wide=True, **kw, **BP)


@pytest.mark.parametrize("q", [4, 64, 256])
@pytest.mark.parametrize("dc", [9, 16, 32])
def test_scaled_check_node_equals_the_brute_force_convolution(q, dc):
    """The statement tests/test_fht32.py makes at degrees up to 8, at degrees 9, 16 and 32: the scaled float32 restatement's c2v against
    the exact box-plus (direct XOR convolution, 80-bit) of the same float32 inputs; every entry whose exact probability is above 2^-12 of
    its vector's largest agrees within a relative 2^-6, and no output lies below -16 ln 2 of its vector's maximum, to float32 rounding
    (log v stays below 39 ln 2 here, so the 2e-5 of that test covers it).  Half the checks carry one flat input."""
    rng = np.random.default_rng(4200 + 1000 * q + dc)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    worst, compared, n = 0.0, 0, 3 if q == 256 else 10
    for k in range(n):
        vin = rng.normal(-2, 4, (dc, q - 1)).astype(np.float32)
        if k % 2:
            vin[int(rng.integers(dc))] = 0.0
        h = rng.integers(1, q, dc)
        got = fw.check_node32_scaled(vin, h, mul)
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        exact = _rel(fr.brute_force(vin, h, mul))
        mine = _rel(got.astype(np.longdouble))
        above = exact > -12 * np.log(2.0)
        worst = max(worst, float(np.max(np.abs(np.expm1(mine - exact))[above])))
        compared += int(above.sum())
        assert float(mine.min()) >= -LN_FLOOR - 2e-5, float(mine.min())
    print(q, dc, "largest relative error above 2^-12:", worst, "= 2^%.1f" % np.log2(max(worst, 1e-300)), "over", compared, "entries")
    assert compared >= n * dc and worst <= 2.0 ** -6


SMALL = [(name, which) for name, _ in CASES for which in SCHEDULES[name]]


@pytest.mark.parametrize("name,which", SMALL, ids=[f"{n}-{w}" for n, w in SMALL])
def test_scaled_equals_unscaled_at_degrees_up_to_eight(oracle, name, which):
    """On every check of every case of tests/test_fht32.py (degrees 2 .. 8), fed the v2c vectors the unscaled restatement gives it in
    every iteration: the transform outputs v of the scaled and the unscaled update are equal bit for bit after division by each vector's
    largest (the scale is a power of two and nothing is subnormal), and their c2v agree within 16 x the case's D32 in the probability
    domain -- they differ only in how log rounds a scaled argument."""
    code, L, iters = fht32_case(name)
    ref = fht32_reference(name, which)
    tol = tolerance(name, which)
    seen = [0, 0.0]

    class Probe(f32.Fht32Check):
        def check(self, m, vin):
            g = self.g
            h = g.c_h[g.coff[m]:g.coff[m + 1]]
            vu, _ = f32.transform_outputs(vin, h, self.mul)
            vs, _, sc = fw.transform_outputs_scaled(vin, h, self.mul)
            assert np.all(sc > 0) and np.all(np.log2(sc.astype(np.float64)) % 1 == 0)
            assert np.array_equal(vu / vu.max(axis=1, keepdims=True), vs / vs.max(axis=1, keepdims=True)), (name, which, m)
            cu, cw = super().check(m, vin), fw.check_node32_scaled(vin, h, self.mul)
            seen[0] += 1
            seen[1] = max(seen[1], fr.w_dev(cu, cw))
            return cu

    base = fht32_checks(name)[0]
    chk = Probe(base.code, base.mul)
    for b in range(L.shape[0]):
        got = fr.decode(chk, L[b], _layer_of(name, which), iters)
        assert np.array_equal(got[4], ref[b][4])            # (the probe is the unscaled restatement, unchanged)
    print(name, which, seen[0], "checks; largest deviation of the c2v", seen[1], "tolerance", tol)
    assert seen[0] > 0 and seen[1] <= tol


def test_flat_inputs_leave_the_range_unscaled_and_stay_inside_it_scaled(oracle):
    """flat-256: a third of the variables flat, 16 of them at the first degree-32 check, exactly one at the first degree-9 check.  At the
    degree-32 check the unscaled tests/fht32_ref.py::check_node32 gives a non-finite value (the product of 16 slots of 256 alone is 2^128);
    the scaled update is finite at every check of every iteration, under both schedules."""
    code, L, iters = cs.case(cs.FLAT)
    flat = cs.flat_set()
    have = cs.flat_per_check(code, flat)
    m32, m9 = int(np.argmax(code.chk_deg == 32)), int(np.argmax(code.chk_deg == 9))
    assert len(flat) == code.N // 3 and have[m32] >= cs.FLAT_IN_32 and have[m9] == 1 and min(have) == 0, have
    assert not L[:, flat].any() and all(L[:, n].all() for n in range(code.N) if n not in flat)
    chk = cs.checks(cs.FLAT)[0]
    g = chk.g
    h = g.c_h[g.coff[m32]:g.coff[m32 + 1]]
    for b in range(L.shape[0]):
        vin = L[b][g.c_var[g.coff[m32]:g.coff[m32 + 1]]].astype(np.float32)      # what the check sees in iteration 1
        with np.errstate(over="ignore", invalid="ignore"):
            try:
                unscaled = f32.check_node32(vin, h, chk.mul)
            except AssertionError:                                               # (its own `t > 0` trips on a NaN maximum)
                unscaled = np.full(1, np.nan)
        assert not np.all(np.isfinite(unscaled)), b
        assert np.all(np.isfinite(fw.check_node32_scaled(vin, h, chk.mul)))
    for which in cs.SCHEDULES:
        for r in cs.reference(cs.FLAT, which):
            assert all(np.all(np.isfinite(r[k])) for k in (3, 4, 5)) and r[4].any()


def test_the_cases_have_the_shapes_they_are_about():
    for name in cs.NAMES:
        code, L, iters = cs.case(name)
        assert code.N <= 96 and code.chk_deg.max() > 8 and iters in (3, 8), name
        assert L.shape[0] == len(cs.kinds(name)) if name != cs.FLAT else L.shape[0] == 2
    code = cs.case(cs.RING)[0]
    assert set(code.chk_deg.tolist()) == {16} and int(nb.layer_greedy(code).max()) + 1 == cs.RING_LAYERS
    for which in cs.SCHEDULES:                               # the ring frames converge at different iterations and never
        flags = [(r[1], r[2]) for r in cs.reference(cs.RING, which)]
        assert flags == [(1, i) if i else (0, 8) for i in cs.RING_ITERS[which]], (which, flags)
        assert len({i for c, i in flags if c}) >= 2 and any(not c for c, _ in flags)
    for name in cs.SW3:
        assert cs.case("sw3:" + name)[0].chk_deg.max() <= 8


ALL_CASES = [(name, which, 0) for name in cs.NAMES + tuple("sw3:" + n for n in cs.SW3) for which in cs.SCHEDULES] + [(cs.RING, which, 1) for which in cs.SCHEDULES]


@pytest.mark.parametrize("name,which,fixed", ALL_CASES, ids=[f"{n}-{w}{'-fixed' if f else ''}" for n, w, f in ALL_CASES])
def test_conditions_on_every_case(oracle, name, which, fixed):
    """Conditions on the inputs alone, for every (case, schedule) tests/test_gpu_fht32_wide.py uses, as
    tests/test_fht32.py::test_conditions_on_every_gpu_case puts them: (a) the two evaluations of the scaled restatement give the same
    out_sym, flags and iteration counts; (b) the smallest decision gap is at least 64 x the largest absolute difference between the two
    over post / v2c entries within 16 of their vector's maximum; (c) D32W, their largest deviation in the probability domain, equals the
    recorded value (to 5 %); (d) 16 x D32W <= 2^-10; (e) the largest |v32 - v80| / t over every check the case evaluates is at most
    2^-18: the floor stays four times above the transform's noise.  The SW3 cases meet (a)-(d) under the unscaled restatement as well
    (D32R).  Largest noise measured over all cases: 2^-19.66 (mix-16, greedy)."""
    pairs = [(cs.reference(name, which, fixed), cs.reference(name, which, fixed, True), fw.D32W[(name + "-fixed" if fixed else name, which)], "D32W")]
    if name.startswith("sw3:"):
        pairs.append((cs.register_reference(name, which), cs.register_reference(name, which, True), cs.D32R[(name, which)], "D32R"))
    for ra, rb, rec, label in pairs:
        dev = 0.0
        for b, (a, x) in enumerate(zip(ra, rb)):
            fig = cs.frame_figures(a, x)
            print(name, which, fixed, label, "frame", b, "same", fig[0], "gap", fig[2], "difference near the top", fig[3], "converged", a[1], "iters", a[2], "dev", fig[4])
            assert cs.frame_ok(fig), (label, b, fig)
            assert np.any(a[4] != 0.0) or a[2] == 1, b
            dev = max(dev, fig[4])
        print(name, which, fixed, label, dev, "recorded", rec, "tolerance", 16 * rec)
        assert 16.0 * dev <= TOL_CAP and 16.0 * rec <= TOL_CAP
        assert abs(dev - rec) <= 0.05 * rec, (label, dev, rec)
    if not fixed:
        worst = max(cs.noise(name, which))
        print(name, which, "largest |v32 - v80| / t = 2^%.2f" % np.log2(worst))
        assert 0.0 < worst <= cs.NOISE_MAX
