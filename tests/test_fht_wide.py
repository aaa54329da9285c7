"""FHT sum-product decoding on codes with checks above degree 8 (nbl_create_fht, check degrees 2 .. 32) without a GPU: the degree limits
of every creation entry point, the plan, the definition (tests/fht_ref.py) against an 80-bit brute-force XOR convolution at those
degrees, and the conditions on the inputs of every case tests/test_gpu_fht_wide.py compares with (tests/fht_wide_cases.py)."""
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import fht_ref as fr
import fht_wide_cases as wc
import layered_bp_ref as lbr
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code, _with_extra_edges
from test_fht import D80_MAX, GAP_MIN, LN_FLOOR, _create_fht
from test_layered import GF16, _refused

BP = dict(method=nb.METHOD_BP, max_iter=5)


def test_header_states_the_limit():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbldpc.h")).read()
    assert "#define NBL_FHT_MAX_CHECK_DEGREE 32" in text
    assert "except the check-degree limit, which is 32 here" in text and "at most 64 KB" in text


def _graphs():
    """a (2, 32)-regular graph; the same with one check of degree 33; checks of degree 8 with one of degree 9; one variable of degree 9
    beside checks of degree 5 at the most; a variable of degree 9 beside a check of degree 33"""
    dc32 = _ring_code(16, 20, 32)
    assert (dc32.chk_deg.min(), dc32.chk_deg.max(), dc32.var_deg.max()) == (32, 32, 2)
    dc33 = _with_extra_edges(dc32, 0, [m for m in range(20) if m not in dc32.var_chk[:2]][:1])
    assert dc33.chk_deg.max() == 33 and dc33.var_deg.max() == 3
    ring8 = _ring_code(16, 12, 8)
    dc9 = _with_extra_edges(ring8, 0, [m for m in range(12) if m not in ring8.var_chk[:2]][:1])
    assert dc9.chk_deg.max() == 9 and dc9.var_deg.max() == 3
    base = _ring_code(16, 12, 4)
    dv9 = _with_extra_edges(base, 0, [m for m in range(12) if m not in base.var_chk[:2]][:7])
    assert dv9.var_deg.max() == 9 and dv9.chk_deg.max() == 5
    both = _with_extra_edges(dc33, 1, [m for m in range(20) if m not in dc33.var_chk[3:5]][:7])
    assert both.var_deg.max() == 9 and both.chk_deg.max() >= 33
    return dc32, dc33, dc9, dv9, both


def test_create_fht_degree_limits_come_before_the_device():
    """nbl_create_fht, both schedules: a check of degree 32 (and of 9) is accepted -- NBL_ERR_NO_DEVICE on a box without a GPU, a decoder on
    one; degree 33 is NBL_ERR_ARG and the text names 32; a variable of degree 9 keeps the text of nbl_create."""
    dc32, dc33, dc9, dv9, both = _graphs()
    for code in (dc32, dc9):
        for layers in (None, "greedy", nb.layer_greedy(code)):
            kw = dict(layers=layers, fht=True, **BP)
            if _no_device():
                _refused(code, -3, "no CPU decode path", **kw)
            else:
                nb.Decoder(code, **kw).close()
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(code), 1)):      # the entry point itself, device -1
            rc, msg = _create_fht(code, lay, flags)
            assert (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg), (rc, msg)
    for layers in (None, "greedy"):
        _refused(dc33, -1, "nbl_create_fht", "check degree 33", "(32)", layers=layers, fht=True, **BP)
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, fht=True, **BP)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, fht=True, **BP)
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(dc33, layers=layers, fht=True, **BP)
        assert "(8)" not in str(e.value)


def test_every_other_entry_point_keeps_its_limit_of_eight():
    """nbl_create, nbl_create_layered, nbl_create_layered_ex and nbl_create_layered_bp: a check of degree 9, 32 or 33 and a variable of
    degree 9 are NBL_ERR_ARG with the text they always had."""
    routes = (dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2),                                   # nbl_create
              dict(method=nb.METHOD_BP, max_iter=5),
              dict(method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=2),
              dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2, layers="greedy"),                  # nbl_create_layered
              dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2, layers="greedy", damped=True),     # nbl_create_layered_ex
              dict(method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=2, layers="greedy", damped=True),
              dict(method=nb.METHOD_BP, max_iter=5, layers="greedy", bp=True))                              # nbl_create_layered_bp
    for code in _graphs():
        for kw in routes:
            with pytest.raises(nb.NblError) as e:
                nb.Decoder(code, **kw)
            assert e.value.status == -1 and str(e.value).endswith("node degree above the supported maximum (8)"), (kw, str(e.value))


def test_plan_names_the_wide_kernels():
    """A code with a check above degree 8 -> fht_wide / fht_wide_layered under every debug switch; force_generic = 3 selects them at any
    degree; every plan of tests/test_fht.py::test_plan_names_the_fht_kernels stays what it was."""
    wide, wide_l = ("fht_wide", False, False, True), ("fht_wide_layered", False, False, True)
    codes = [wc.wide_case(name)[0] for name in wc.NAMES] + [_ring_code(16, 20, 32), _graphs()[2]]
    for code in codes:
        assert code.chk_deg.max() > 8
        for fg, rs in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
            assert debug_plan(code, nb.METHOD_BP, fht=True, force_generic=fg, record_state=rs) == wide
            assert debug_plan(code, nb.METHOD_BP, fht=True, layers="greedy", force_generic=fg, record_state=rs) == wide_l
    small = [profile_code("all", q)[0] for q in (4, 8, 16, 32, 64, 128, 256)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4),
                                                                                  _ring_code(256, 12, 8)]
    for code in small:
        assert code.chk_deg.max() <= 8
        for rs in (False, True):
            assert debug_plan(code, nb.METHOD_BP, fht=True, force_generic=3, record_state=rs) == wide
            assert debug_plan(code, nb.METHOD_BP, fht=True, layers="greedy", force_generic=3, record_state=rs) == wide_l
        for fg, rs in ((0, False), (1, False), (2, False), (0, True)):
            assert debug_plan(code, nb.METHOD_BP, fht=True, force_generic=fg, record_state=rs) == ("fht", False, False, True)
            assert debug_plan(code, nb.METHOD_BP, fht=True, layers="greedy", force_generic=fg, record_state=rs) == ("fht_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP, layers="greedy") == ("bp_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP)[0] in ("bp256", "bp64", "bp_small", "bp")
        assert debug_plan(code, nb.METHOD_BP, force_generic=1)[0] == "bp"


def _bpsk_vectors(rng, q, dc, ebn0_db=5.0):
    """symbol LLRs of all-zero BPSK symbols at the rate of a (2, dc)-regular code, (dc - 2) / dc: a high-rate operating point"""
    p = q.bit_length() - 1
    sigma = 1.0 / np.sqrt(2 * ((dc - 2) / dc) * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((dc, p))) / sigma ** 2
    a = np.arange(1, q)
    return bit @ ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64).T


@pytest.mark.parametrize("kind,tol", [("normal", 1e-9), ("bpsk", 1e-5)])
@pytest.mark.parametrize("q,dc", [(16, 32), (64, 24), (256, 16), (256, 32)])
def test_check_node_equals_the_brute_force_convolution_at_high_degrees(q, dc, kind, tol):
    """tests/test_fht.py::test_check_node_equals_the_brute_force_convolution at check degrees 16, 24 and 32, with its tolerances: every
    entry more than one nat above the floor agrees with the exact box-plus (direct XOR convolution, 80-bit) to `tol`, and every vector
    decides the same.  3 checks each.  Measured: 3.9e-15 (normal) / 4.9e-11 (BPSK at 5 dB, the worst at q = 256, dc = 16).  A property of the definition, not of a kernel."""
    rng = np.random.default_rng(1000 * q + dc)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    worst, compared = 0.0, 0
    for _ in range(3):
        vin = rng.normal(-2, 4, (dc, q - 1)) if kind == "normal" else _bpsk_vectors(rng, q, dc)
        h = rng.integers(1, q, dc)
        got, exact = wc.check_node(vin, h, mul), fr.brute_force(vin, h, mul)
        above = exact > np.maximum(exact.max(axis=1, keepdims=True), 0.0) - LN_FLOOR + 1.0
        worst = max(worst, float(np.max(np.abs(got - exact)[above])))
        compared += int(above.sum())
        for d in range(dc):
            assert lbr._decide(got[d]) == lbr._decide(np.asarray(exact[d], dtype=np.float64)), d
        assert np.all(got >= np.maximum(got.max(axis=1, keepdims=True), 0.0) - LN_FLOOR - 1e-9)   # nothing below the floor
    print(q, dc, kind, "largest |c2v - exact| above the floor:", worst, "over", compared, "entries")
    assert compared > 3 * dc and worst <= tol


def test_the_cases_have_the_degrees_they_are_about():
    for name in wc.NAMES:
        code = wc.wide_case(name)[0]
        if name.startswith("wide"):
            assert sorted(set(code.chk_deg.tolist())) == [9, 12, 16, 17, 24, 32] and code.N == 88, name
        elif name.startswith("mix"):
            assert sorted(set(code.chk_deg.tolist())) == [2, 3, 4, 8, 9, 10, 31, 32] and sorted(set(code.var_deg.tolist())) == [1, 2, 3, 8] and code.N == 54, name
        else:
            assert set(code.chk_deg.tolist()) == {16} and set(code.var_deg.tolist()) == {2} and (code.N, code.M) == (96, 12)
            assert int(nb.layer_greedy(code).max()) + 1 == wc.RING_LAYERS
        assert code.N <= 96


WIDE_CASES = [(name, which, 0) for name in wc.NAMES for which in wc.SCHEDULES] + [(wc.RING, which, 1) for which in wc.SCHEDULES]


@pytest.mark.parametrize("name,which,fixed", WIDE_CASES, ids=[f"{n}-{w}{'-fixed' if f else ''}" for n, w, f in WIDE_CASES])
def test_conditions_on_every_wide_case(oracle, name, which, fixed):
    """The conditions of tests/test_fht.py::test_conditions_on_every_gpu_case on every case tests/test_gpu_fht_wide.py uses: (a) the
    smallest decide gap is at least 1e-6, (b) the FP64 and the 80-bit restatement give the same out, converged and iters, (c) their
    states differ by at most 1e-10 in the probability domain; the figure of (c) is the one recorded in fht_wide_cases.D80."""
    r64, r80 = wc.wide_reference(name, which, fixed), wc.wide_reference80(name, which, fixed)
    d80 = 0.0
    for b, (a, x) in enumerate(zip(r64, r80)):
        d = fr.state_dev(a, x)
        print(name, which, fixed, b, "gap", a[6], "converged", a[1], "iters", a[2], "D80", d)
        assert min(a[6], x[6]) >= GAP_MIN, (b, a[6], x[6])
        assert np.array_equal(a[0], x[0]) and (a[1], a[2]) == (x[1], x[2]), b
        assert all(np.all(np.isfinite(a[k])) for k in (3, 4, 5)) and (np.any(a[4] != 0.0) or a[2] == 1), b
        d80 = max(d80, d)
    rec = wc.D80[(name + "-fixed" if fixed else name, which)]
    print(name, which, fixed, "D80", d80, "recorded", rec)
    assert d80 <= D80_MAX and rec <= D80_MAX
    assert abs(d80 - rec) <= 0.05 * rec, (d80, rec)
    if name == wc.RING:
        want = [(1, i) if i else (0, 8) for i in wc.RING_ITERS[which]]
        assert [(r[1], r[2]) for r in r64] == want, [(r[1], r[2]) for r in r64]
