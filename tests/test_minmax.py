"""Min-Max decoding (method 3, nbl_create_minmax) without a GPU: the recursion of tests/minmax_ref.py against the brute-force minimum over
all configurations, bit for bit; the conditions every case of tests/test_gpu_minmax.py must meet (tests/minmax_cases.py); the refusals of
the entry point, each by status and message, all before the device; nbl_create's own refusal of method 3; the header, the export, the plan
names and the LDS figure."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nbldpc_amd as nb
import minmax_cases as mc
import minmax_ref as mr
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_fht_wide import _graphs
from test_layered import GF16, _refused

MM = dict(method=nb.METHOD_MINMAX, max_iter=5, minmax=True)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(code, layer_of, flags, method=nb.METHOD_MINMAX, factor=1.0, gf=None):
    """nbl_create_minmax itself, device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in (gf if gf is not None else nb.datafiles.gf_tables(code.q)))
    prm = nb.binding.Params(method, 5, 4, 2, factor, 0.0, 2, 2, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_minmax(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def _past_every_check(rc, msg):
    """what an accepted request gives with device -1: no device at all, or an index out of range"""
    return (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg)


def lds_bytes(q, maxdc):
    """the library's own figure: the function both launchers size by"""
    fn = nb.load_library().nbl_debug_minmax_lds_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_int32] * 2
    return int(fn(q, maxdc))


# ---- 1. the recursion is the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,dc", [(4, 2), (4, 3), (4, 5), (8, 4), (16, 3)])
def test_the_recursion_equals_the_minimum_over_all_configurations(q, dc):
    """Step 3 of the header is a definition by set; the forward / backward recursion evaluates it exactly.  Every output edge, with and
    without shaping, bit for bit; inputs with ties (a quantised vector) and with an all-negative vector (maximum at slot 0) among them."""
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    rng = np.random.default_rng(100 * q + dc)
    for trial in range(4):
        vin = rng.normal(-1.0, 4.0, (dc, q - 1))
        if trial == 1:
            vin = np.round(vin)                                               # ties between entries and between edges
        if trial == 2:
            vin[0] = -np.abs(vin[0]) - 0.5                                     # m_0 = 0: the maximum is the slot 0
        h = rng.integers(1, q, dc)
        u = mr.dissimilarities(vin, h, mul)
        assert (u >= 0).all() and (u.min(axis=1) == 0).all()
        w, wb = mr.combine(u), mr.combine_brute(u)
        assert w.shape == (dc, q) and np.array_equal(w, wb), (q, dc, trial)
        for kw in ({}, dict(factor=1.1, offset=0.1), dict(factor=1.0, offset=0.25)):
            a, b = mr.check_node(vin, h, mul, **kw), mr.check_node(vin, h, mul, brute=True, **kw)
            assert a.shape == (dc, q - 1) and np.array_equal(a, b), (q, dc, trial, kw)
        assert (mr.check_node(vin, h, mul) <= 0).any() and np.isfinite(mr.check_node(vin, h, mul)).all()


def test_shaping_is_the_identity_the_division_and_the_dead_zone():
    y = np.array([-3.0, -0.05, 0.0, 0.05, 2.2])
    assert np.array_equal(mr.shape(y, 1.0, 0.0), y)
    assert np.array_equal(mr.shape(y, 1.1, 0.1), [-3.0 / 1.1 + 0.1, 0.0, 0.0, 0.0, 2.2 / 1.1 - 0.1])
    assert np.array_equal(mr.shape(y, 1.0, 0.1), [-2.9, 0.0, 0.0, 0.0, 2.2 - 0.1])


# ---- 2. the conditions on the GPU cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.NAMES)
def test_every_case_has_the_convergence_spread_under_both_schedules(name):
    """under each schedule at least one frame never converges within MAX_ITER, one converges after iteration 1 and one at iteration 1; the
    two schedules differ in c2v, so a schedule bit that is ignored cannot pass"""
    refs = {which: mc.reference(name, which) for which in mc.SCHEDULES}
    for which, ref in refs.items():
        never, later, first = mc.spread(ref)
        print(name, which, [r[2] if r[1] else 0 for r in ref])
        assert never >= 1 and later >= 1 and first >= 1, (name, which, never, later, first)
        assert len(ref) == len(mc.LEVELS) and all(np.isfinite(r[3]).all() and np.isfinite(r[4]).all() for r in ref)
    assert any(not np.array_equal(a[4], b[4]) for a, b in zip(refs["flooding"], refs["greedy"])), name
    greedy = mc.layer_of(name, "greedy")
    assert int(greedy.max()) + 1 > 1, name                                    # (one layer would be the flooding schedule)


def test_recorded_iteration_counts():
    """the counts the cases were chosen by (0 = never)"""
    want = {("wide16", "flooding"): [0, 0, 2, 2, 1, 1], ("mix4", "flooding"): [0, 3, 3, 2, 1, 1], ("mix4", "greedy"): [0, 3, 2, 2, 1, 1],
            ("wide256", "flooding"): [0, 0, 2, 2, 1, 1]}
    for (name, which), counts in want.items():
        assert [r[2] if r[1] else 0 for r in mc.reference(name, which)] == counts, (name, which)


def test_realised_degree_sets():
    from fht_wide_cases import MIX_DEGS, WIDE_DEGS
    degs = {name: (set(mc.case(name)[0].chk_deg.tolist()), set(mc.case(name)[0].var_deg.tolist())) for name in mc.NAMES}
    for name in ("wide16", "wide64"):
        assert degs[name] == (set(WIDE_DEGS[0]), set(WIDE_DEGS[1])), name
    for name in ("mix4", "mix128"):
        assert degs[name][0] == set(MIX_DEGS[0]) == {2, 3, 4, 8, 9, 10, 31, 32} and {1, 8} <= degs[name][1], name
    assert degs["wide256"] == ({9, 16, 32}, {2, 3}) and degs["shaped16"] == ({9, 10}, {2, 3})
    assert degs["ring256-dc4"] == ({4}, {2}) and mc.case("ring256-dc4")[0].N == 16
    assert mc.case("shaped16")[1] == dict(ems_factor=1.1, ems_offset=0.1)
    # waves per check 1 / 2 / 4, and an edge count the wave count does not divide at two and at four waves
    assert {mc.case(n)[0].q for n in mc.NAMES} == {4, 16, 64, 128, 256}
    assert any(d % 2 for d in degs["mix128"][0]) and any(d % 4 for d in degs["wide256"][0])


# ---- 3. refusals, all before the device -------------------------------------------------------------------------------------------------
def test_accepted_requests_pass_every_check():
    dc32 = _graphs()[0]
    for code in (dc32, _ring_code(256, 20, 32), nb.Code(GF16), mc.case("mix4")[0]):
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(code), 1)):
            assert _past_every_check(*_create(code, lay, flags)), (lay, flags)
        for layers in (None, "greedy"):
            if _no_device():
                _refused(code, -3, "no CPU decode path", layers=layers, **MM)


def test_refusals_of_method_flags_and_layers():
    dc32 = _graphs()[0]
    for code in (dc32, nb.Code(GF16)):
        for method, extra in ((nb.METHOD_EMS, dict(ems_nm=4, ems_nc=2)), (nb.METHOD_BP, {}), (nb.METHOD_TEMS, {}), (nb.METHOD_BS_TEMS, {}), (nb.METHOD_OSD, {}),
                              (5, {}), (0, {})):
            for layers in (None, "greedy"):
                _refused(code, -2, "nbl_create_minmax", "(method 3)", method=method, max_iter=5, layers=layers, minmax=True, **extra)
            rc, msg = _create(code, None, 0, method=method)
            assert rc == -2 and "nbl_create_minmax" in msg and "(method 3)" in msg, (method, rc, msg)
        for flags in (2, 3, 0x80000000):
            rc, msg = _create(code, None, flags)
            assert rc == -1 and "nbl_create_minmax" in msg and "unknown flag bit" in msg and "NBL_MINMAX_LAYERED" in msg, (flags, rc, msg)
        rc, msg = _create(code, nb.layer_greedy(code), 0)
        assert rc == -1 and "nbl_create_minmax" in msg and "layer_of = NULL" in msg, (rc, msg)
    # the Python class refuses the options the entry point has no argument for, and the other kinds beside it
    for kw in (dict(osd_order=0), dict(bs_nm=4), dict(layers="greedy", damped=True), dict(layers="greedy", bp=True), dict(fht=True), dict(wide=True),
               dict(tems_wide=True), dict(bp_wide=True), dict(fht32=True), dict(fht32_wide=True)):
        with pytest.raises(ValueError):
            nb.Decoder(dc32, **MM, **kw)
    for kw in (dict(fht=True), dict(wide=True), dict(tems_wide=True), dict(bp_wide=True), dict(fht32=True), dict(fht32_wide=True)):
        with pytest.raises(ValueError):
            debug_plan(dc32, nb.METHOD_MINMAX, minmax=True, **kw)


def test_degree_field_and_parameter_limits():
    dc32, dc33, dc9, dv9, both = _graphs()
    for layers in (None, "greedy"):
        _refused(dc33, -1, "nbl_create_minmax", "check degree 33 ", "(32)", layers=layers, **MM)
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(dc33, layers=layers, **MM)
        assert "(8)" not in str(e.value)
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, **MM)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, **MM)
        _refused(_ring_code(512, 8, 4), -2, "GF(256)", layers=layers, gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **MM)
        _refused(dc32, -1, "nbl_create_minmax", "ems_factor", layers=layers, ems_factor=0.0, **MM)
    rc, msg = _create(dc32, None, 0, factor=0.0)
    assert rc == -1 and "nbl_create_minmax" in msg and "ems_factor" in msg, (rc, msg)
    # a bad field table: the text of nbl_create
    mul, inv = nb.datafiles.gf_tables(16)
    mul = [row[:] for row in mul]
    mul[3][4], mul[3][5] = mul[3][5], mul[3][4]
    _refused(dc32, -1, "gf_mul[3][4]", "not a polynomial-basis", gf=(mul, inv), **MM)
    rc, msg = _create(dc32, None, 1, gf=(mul, inv))
    assert rc == -1 and "gf_mul[3][4]" in msg, (rc, msg)
    # everything else nbl_create refuses, with its text
    _refused(dc32, -1, "max_iter < 0", method=nb.METHOD_MINMAX, max_iter=-1, minmax=True)
    broken = _ring_code(16, 20, 32)
    broken.chk_h = broken.chk_h.copy()
    broken.chk_h[2] = 0
    _refused(broken, -1, "zero coefficient", **MM)


def test_every_layer_assignment_error_keeps_the_text_of_nbl_create_layered():
    """The assignment errors of tests/test_layered.py, on the shipped GF(16) code and on a degree-32 graph: status and text are those
    nbl_create_layered gives where it accepts the graph."""
    for code in (nb.Code(GF16), _graphs()[0]):
        greedy = nb.layer_greedy(code)
        off = np.concatenate([[0], np.cumsum(code.chk_deg)])
        v = int(code.chk_var[0])
        other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
        shared = greedy.copy()
        shared[other] = shared[0]
        shared = np.unique(shared, return_inverse=True)[1].reshape(-1).astype(np.int32)   # (no layer left empty: that error would come first)
        first = next((m, int(x)) for m in range(code.M) for x in code.chk_var[off[m]:off[m + 1]]
                     if any(shared[k] == shared[m] and int(x) in code.chk_var[off[k]:off[k + 1]].tolist() for k in range(m)))
        partner = next(k for k in range(first[0]) if shared[k] == shared[first[0]] and first[1] in code.chk_var[off[k]:off[k + 1]].tolist())
        below, gap, far = greedy.copy(), greedy.copy(), greedy.copy()
        below[3] = -1
        gap[gap == gap.max()] += 1
        far[5] = 1 << 30
        for layers, words in ((shared, (f"checks {partner} and {first[0]} ", f"share variable {first[1]}")), (below, ("layer_of[3]", "below 0")),
                              (gap, ("layered schedule", "empty"), ), (far, ("empty layer",))):
            _refused(code, -1, *words, layers=layers, **MM)
            rc, msg = _create(code, layers, 1)
            assert rc == -1 and all(w in msg for w in words), (rc, msg)
            if code.chk_deg.max() <= 8:
                with pytest.raises(nb.NblError) as e:
                    nb.Decoder(code, nb.METHOD_EMS, 5, ems_nm=4, ems_nc=2, layers=layers)
                assert msg in str(e.value), (str(e.value), msg)


# ---- 4. method 3 without the flag -------------------------------------------------------------------------------------------------------
def test_method_3_outside_nbl_create_minmax_is_refused_as_before():
    text = "decode method not supported (reference: 'has not been developed')"
    for code in (nb.Code(GF16), _graphs()[0]):
        _refused(code, -2, text, method=3, max_iter=5)
        _refused(code, -2, method=3, max_iter=5, osd_order=0)
        _refused(code, -2, method=3, max_iter=5, bs_nm=4)
    code = nb.Code(GF16)
    _refused(code, -2, "the layered schedule is defined for EMS (method 2) only", method=3, max_iter=5, layers="greedy")
    _refused(code, -2, method=3, max_iter=5, layers="greedy", damped=True)
    _refused(code, -2, "nbl_create_layered_bp runs log-QSPA (method 1) only", method=3, max_iter=5, layers="greedy", bp=True)
    for kind in ("fht", "wide", "tems_wide", "bp_wide", "fht32", "fht32_wide"):
        _refused(code, -2, method=3, max_iter=5, **{kind: True})


# ---- 5. header and export ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_macros_and_the_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "nbldpc.h")).read()
    for line in ("#define NBL_METHOD_MINMAX 3", "#define NBL_MINMAX_LAYERED 1u", "#define NBL_MINMAX_MAX_CHECK_DEGREE 32"):
        assert line in text, line
    assert "nbl_create_minmax" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_minmax")
    assert nb.METHOD_MINMAX == 3 and nb.MINMAX_LAYERED == 1
    assert "method 3 outside nbl_create_minmax" in text


# ---- 6. the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_names_minmax_at_every_degree_under_every_switch():
    codes = [_ring_code(16, 8, 4), _ring_code(256, 8, 4), _ring_code(16, 20, 32), _ring_code(256, 20, 32), nb.Code(GF16)] + [mc.case(n)[0] for n in mc.NAMES]
    for code in codes:
        for fg in (0, 1, 2, 3):
            for rs in (False, True):
                assert debug_plan(code, nb.METHOD_MINMAX, minmax=True, force_generic=fg, record_state=rs) == ("minmax", False, False, True)
                assert debug_plan(code, nb.METHOD_MINMAX, minmax=True, layers="greedy", force_generic=fg, record_state=rs) == ("minmax_layered", False, False, False)
    assert {int(c.chk_deg.max()) for c in codes} >= {4, 32}


# ---- 7. LDS -----------------------------------------------------------------------------------------------------------------------------
def test_lds_figure_is_the_headers():
    """[maxdc][q] dissimilarities, two [q] operand blocks, two [q] output vectors: (maxdc + 4) q 8 bytes; below 160 KB for every shape the
    ABI accepts, so creation refuses no shape for LDS.  The header quotes the figure at q = 256, degree 32."""
    for q in (4, 8, 16, 32, 64, 128, 256):
        for dc in range(2, 33):
            assert lds_bytes(q, dc) == (dc + 4) * q * 8 <= 160 * 1024, (q, dc)
    text = open(os.path.join(ROOT, "include", "nbldpc.h")).read()
    sect = text[text.index("Min-Max decoding (method 3)"):text.index("#define NBL_METHOD_MINMAX")]
    m = re.search(r"at most ([0-9,]+) at q = 256 and degree 32", sect)
    assert m and int(m.group(1).replace(",", "")) == lds_bytes(256, 32) == 73728 > 64 * 1024   # (the launchers opt in above 64 KB)
