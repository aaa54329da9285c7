"""EMS decoding on codes with checks above degree 8 (nbl_create_ems_wide, check degrees 2 .. 32) without a GPU: the limits of the entry
point, all before the device; the plan; the oracle pinned to the compiled reference at these degrees (the deg_wide_* fixtures of
tests/golden/make_golden_ems_wide.py); and the conditions on the inputs of every case tests/test_gpu_ems_wide.py compares with
(tests/ems_wide_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import ems_wide_cases as wc
import test_oracle_golden as tog
from conftest import load_golden
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_fht_wide import _graphs
from test_layered import GF16, _refused

EMS = dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2)
WIDE_SETS = ["deg_wide_gf64_ems", "deg_wide_gf16_ems", "deg_wide_gf256_ems"]
MAX_LDS = 160 * 1024


def _create_wide(code, layer_of, flags, ems_nm=4, ems_nc=2, method=nb.METHOD_EMS):
    """nbl_create_ems_wide itself, device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in nb.datafiles.gf_tables(code.q))
    prm = nb.binding.Params(method, 5, ems_nm, ems_nc, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_ems_wide(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def _past_every_check(rc, msg):
    """what an accepted request gives with device -1: no device at all, or an index out of range"""
    return (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg)


def lds_bytes(q, maxdc, nm, nc):
    """the library's own figure: the function creation's refusal and both launchers use"""
    fn = nb.load_library().nbl_debug_ems_wide_lds_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_int32] * 4
    return int(fn(q, maxdc, nm, nc))


def test_header_states_the_limit_and_the_library_exports_the_entry_point():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbldpc.h")).read()
    assert "#define NBL_EMS_MAX_CHECK_DEGREE 32" in text and "#define NBL_EMS_WIDE_LAYERED 1u" in text
    assert "nbl_create_ems_wide" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_ems_wide")


def test_create_ems_wide_degree_limits_come_before_the_device():
    """Both schedules: a check of degree 32 (and of 9) is accepted -- NBL_ERR_NO_DEVICE on a box without a GPU, a decoder on one; degree
    33 is NBL_ERR_ARG and the text names the entry point, 33 and 32, not "(8)"; a variable of degree 9 keeps the text of nbl_create."""
    dc32, dc33, dc9, dv9, both = _graphs()
    for code in (dc32, dc9):
        for layers in (None, "greedy", nb.layer_greedy(code)):
            kw = dict(layers=layers, wide=True, **EMS)
            if _no_device():
                _refused(code, -3, "no CPU decode path", **kw)
            else:
                nb.Decoder(code, **kw).close()
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(code), 1)):
            assert _past_every_check(*_create_wide(code, lay, flags)), (lay, flags)
    for layers in (None, "greedy"):
        _refused(dc33, -1, "nbl_create_ems_wide", "check degree 33", "(32)", layers=layers, wide=True, **EMS)
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, wide=True, **EMS)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, wide=True, **EMS)
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(dc33, layers=layers, wide=True, **EMS)
        assert "(8)" not in str(e.value)


def test_create_ems_wide_refusals_of_method_flags_and_layers():
    dc32 = _graphs()[0]
    for code in (dc32, nb.Code(GF16)):
        for method, extra in ((nb.METHOD_BP, {}), (nb.METHOD_TEMS, dict(tems_nr=2, tems_nc=2)), (nb.METHOD_BS_TEMS, {})):
            for layers in (None, "greedy"):
                _refused(code, -2, "nbl_create_ems_wide", "(method 2)", method=method, max_iter=5, layers=layers, wide=True, **extra)
        for flags in (2, 3, 0x80000000):
            rc, msg = _create_wide(code, None, flags)
            assert rc == -1 and "unknown flag bit" in msg and "NBL_EMS_WIDE_LAYERED" in msg, (flags, rc, msg)
        rc, msg = _create_wide(code, nb.layer_greedy(code), 0)
        assert rc == -1 and "nbl_create_ems_wide" in msg and "layer_of = NULL" in msg, (rc, msg)
        # an invalid assignment keeps nbl_create_layered's status and text
        bad, texts = np.zeros(code.M, dtype=np.int32), []
        for kw in (dict(), dict(wide=True)):
            if kw or code.chk_deg.max() <= 8:                       # (nbl_create_layered itself refuses the degree-32 graph first)
                with pytest.raises(nb.NblError) as e:
                    nb.Decoder(code, layers=bad, **EMS, **kw)
                assert e.value.status == -1 and "layered schedule: checks" in str(e.value) and "share variable" in str(e.value), str(e.value)
                texts.append(str(e.value))
        assert len(set(texts)) == 1, texts
    # everything else nbl_create refuses: nm above q, with the reference's text
    _refused(dc32, -1, "EMS_Nm is too large", method=nb.METHOD_EMS, max_iter=5, ems_nm=17, ems_nc=2, wide=True)
    # the Python class refuses the options the entry point has no argument for
    for kw in (dict(osd_order=0), dict(bs_nm=4), dict(layers="greedy", damped=True), dict(layers="greedy", bp=True), dict(fht=True)):
        with pytest.raises(ValueError):
            nb.Decoder(dc32, wide=True, **EMS, **kw)


def test_lds_size_function_and_its_refusal():
    """[maxdc][q] inputs, three [layers][q] DP arrays, one [q] vector, the lists [maxdc][nm] at 8 + 4 bytes (+ 16): the library's figure is
    that formula; a shape it puts above 160 KB is NBL_ERR_UNSUPPORTED with the byte count in the text, the one just below is accepted."""
    def formula(q, maxdc, nm, nc):
        layers = 1 if nc >= maxdc - 1 else nc + 1
        return (maxdc * q + 3 * layers * q + q + maxdc * nm) * 8 + maxdc * nm * 4 + 16
    for shape in ((256, 32, 32, 3), (256, 32, 256, 3), (64, 32, 16, 3), (16, 10, 4, 9), (16, 10, 4, 0), (4, 2, 4, 1), (128, 17, 8, 2)):
        assert lds_bytes(*shape) == formula(*shape), shape
    assert lds_bytes(256, 32, 32, 3) == 104464                      # the shape of the issue's occupancy argument: one workgroup per CU
    assert lds_bytes(256, 32, 256, 3) > MAX_LDS                     # nm = q = 256 at degree 32
    assert lds_bytes(256, 32, 186, 3) <= MAX_LDS < lds_bytes(256, 32, 187, 3)
    code = _ring_code(256, 20, 32)
    assert code.chk_deg.max() == 32
    for flags in (0, 1):
        assert _past_every_check(*_create_wide(code, None, flags, ems_nm=186, ems_nc=3)), flags
        for nm in (187, 256):
            rc, msg = _create_wide(code, None, flags, ems_nm=nm, ems_nc=3)
            assert rc == -2 and "nbl_create_ems_wide" in msg and str(lds_bytes(256, 32, nm, 3)) in msg and "LDS" in msg, (rc, msg)


def test_plan_names_the_wide_kernels():
    """A code with a check above degree 8 -> ems_wide / ems_wide_layered under every debug switch; a code without one gets the plan of
    nbl_create / nbl_create_layered, fused kernels included, unless force_generic is 3."""
    kw = dict(ems_nm=4, ems_nc=2)
    codes = [wc.wide_case(name)[0] for name in wc.NAMES] + [_ring_code(16, 20, 32), _graphs()[2]]
    for code in codes:
        assert code.chk_deg.max() > 8
        for fg, rs in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
            assert debug_plan(code, nb.METHOD_EMS, wide=True, force_generic=fg, record_state=rs, **kw) == ("ems_wide", False, False, True)
            assert debug_plan(code, nb.METHOD_EMS, wide=True, layers="greedy", force_generic=fg, record_state=rs, **kw) == ("ems_wide_layered", False, False, False)
    small = [profile_code("all", q)[0] for q in (4, 8, 16, 32, 64, 128, 256)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4),
                                                                                  _ring_code(128, 12, 8), _ring_code(256, 12, 8)]
    names = set()
    for code in small:
        assert code.chk_deg.max() <= 8
        for nm_nc in (dict(ems_nm=4, ems_nc=2), dict(ems_nm=min(32, code.q), ems_nc=3)):
            for fg, rs in ((0, False), (1, False), (2, False), (0, True), (2, True)):
                plain = debug_plan(code, nb.METHOD_EMS, force_generic=fg, record_state=rs, **nm_nc)
                assert debug_plan(code, nb.METHOD_EMS, wide=True, force_generic=fg, record_state=rs, **nm_nc) == plain
                names.add(plain[0])
                plain = debug_plan(code, nb.METHOD_EMS, layers="greedy", force_generic=fg, record_state=rs, **nm_nc)
                assert plain[0] == "ems_layered"
                assert debug_plan(code, nb.METHOD_EMS, wide=True, layers="greedy", force_generic=fg, record_state=rs, **nm_nc) == plain
            for rs in (False, True):
                fusable = debug_plan(code, nb.METHOD_EMS, **nm_nc)[1]
                assert debug_plan(code, nb.METHOD_EMS, wide=True, force_generic=3, record_state=rs, **nm_nc) == ("ems_wide", fusable, False, True)
                assert debug_plan(code, nb.METHOD_EMS, wide=True, layers="greedy", force_generic=3, record_state=rs, **nm_nc) == ("ems_wide_layered", False, False, False)
            # the switch means nothing to a decoder of nbl_create
            assert debug_plan(code, nb.METHOD_EMS, force_generic=3, **nm_nc)[0] in ("ems256", "ems_small", "ems64", "ems")
    assert {"ems256", "ems"} <= names, names


@pytest.mark.parametrize("name", WIDE_SETS)
def test_wide_fixtures_literal_bit_exact(oracle, name):
    """The literal oracle equals the compiled reference bit for bit on checks of degree 9 .. 32: out, ret and syn_ok of every frame at
    every recorded iteration count, post / v2c / c2v of the recorded frame."""
    g, meta = load_golden(name)
    assert meta["profile"]["method"] == 2 and min(meta["chk_degs"]) >= 9
    assert meta["chk_degs"] == ([9, 12, 16, 17] if name == "deg_wide_gf256_ems" else [9, 12, 16, 17, 24, 32])
    flags = g["syn_ok"][-1].tolist()
    assert 0 in flags and 1 in flags and g["syn_ok"][0].any() and not g["syn_ok"][0].all()      # at once, later and never
    tog._check_fixture(oracle, g, meta, name, oracle.LITERAL, True)


@pytest.mark.parametrize("name", WIDE_SETS)
def test_wide_fixtures_canonical_matches_reference_decisions(oracle, name):
    """The canonical oracle gives the compiled reference's decisions, flags and iteration counts on every frame; its state differs by the
    reference's add-then-subtract residue only, held to the tolerance tests/test_oracle_golden.py applies to deg_dc78_gf64_ems
    (measured: 9.9e-12 absolute at GF(64), 1.3e-11 at GF(16) shaped, 2.4e-12 at GF(256))."""
    g, meta = load_golden(name)
    tog._check_fixture(oracle, g, meta, name, oracle.CANONICAL, False)
    gap = 0.0
    for k, it in enumerate(g["state_iters"]):
        dec = tog._mk_deg(oracle, meta, it, oracle.CANONICAL)
        dec.decode(g["L_ch"][int(g["state_lanes"][0])])
        for a, ref in zip(dec.state(), (g["st_post"][k, 0], g["st_v2c"][k, 0], g["st_c2v"][k, 0])):
            gap = max(gap, float(np.max(np.abs(a - ref))))
    print(name, "largest |canonical - reference| over the recorded state:", gap)


def test_the_cases_have_the_degrees_they_are_about():
    want = {"gf64-nm8": [9, 12, 16, 17, 24, 32], "gf64-nm16": [9, 12, 16, 17, 24, 32], "gf16-shaped": [9, 12, 16, 17, 24, 32], "gf4-full": [9, 12, 16, 17, 24, 32],
            "gf256-dc17": [9, 12, 16, 17], "gf256-nm12": [9, 16, 32], "gf128-mix": [2, 3, 4, 8, 9, 10, 31, 32], "gf16-nc9": [9, 10], "gf16-nc0": [9, 10]}
    assert set(want) == set(wc.NAMES)
    for name in wc.NAMES:
        code, kw, L = wc.wide_case(name)
        assert sorted(set(code.chk_deg.tolist())) == want[name] and code.N <= 88 and L.shape[0] <= wc.B_BATCH, name
        assert sorted(set(code.var_deg.tolist())) == ([1, 2, 3, 8] if name == "gf128-mix" else [2, 3]), name
        assert lds_bytes(code.q, int(code.chk_deg.max()), kw["ems_nm"], kw["ems_nc"]) <= MAX_LDS
    assert wc.wide_case("gf4-full")[1]["ems_nm"] == 4 and wc.wide_case("gf256-nm12")[1]["ems_nm"] & (wc.wide_case("gf256-nm12")[1]["ems_nm"] - 1)
    assert wc.wide_case("gf16-nc9")[1]["ems_nc"] >= 10 - 1            # nc >= dc - 1: no deviation counting


@pytest.mark.parametrize("fixed", [0, 1])
@pytest.mark.parametrize("which", wc.SCHEDULES)
@pytest.mark.parametrize("name", wc.NAMES)
def test_conditions_on_every_gpu_case(oracle, name, which, fixed):
    """Under the canonical oracle at least one frame of the case converges at iteration 1, at least one later and at least one never
    within MAX_ITER; no decision is a tie; some check node ran.  Fixed iterations freeze the same outputs at the same counts."""
    ref = wc.wide_reference(name, which, fixed)
    flags = [(r[1], r[2]) for r in ref]
    print(name, which, fixed, flags, "smallest margin", min(wc.margin(r[3]) for r in ref))
    assert (1, 1) in flags and any(c and 1 < i <= wc.MAX_ITER for c, i in flags) and (0, wc.MAX_ITER) in flags, flags
    for b, r in enumerate(ref):
        assert wc.margin(r[3]) > 0.0, (name, which, b)
        assert np.all(np.isfinite(r[3])) and np.all(np.isfinite(r[4])), b
        assert r[4].any() or (r[2] == 1 and not fixed), b
    if fixed:
        early = wc.wide_reference(name, which, 0)
        assert [(r[1], r[2]) for r in early] == flags and all(np.array_equal(a[0], b[0]) for a, b in zip(ref, early))
