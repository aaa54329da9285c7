"""Exact log-QSPA on codes with checks above degree 8 (nbl_create_bp_wide, check degrees 2 .. 32) without a GPU: the limits and refusals of
the entry point, all before the device; the plan; the LDS figure; the oracle pinned to the compiled reference at these degrees (the
deg_wide_*_bp fixtures of tests/golden/make_golden_bp_wide.py); the flooding restatement of tests/bp_wide_ref.py against the oracle's own
decoder; and the margin condition on the inputs of every case tests/test_gpu_bp_wide.py compares with (tests/bp_wide_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import bp_wide_cases as bc
import bp_wide_ref
import test_oracle_golden as tog
from conftest import load_golden
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_fht_wide import _graphs
from test_layered import GF16, _refused

BP = dict(method=nb.METHOD_BP, max_iter=5)
WIDE_SETS = ["deg_wide_gf16_bp", "deg_wide_gf64_bp", "deg_wide_gf256_bp"]
MAX_LDS = 160 * 1024


def _create_wide(code, layer_of, flags, method=nb.METHOD_BP):
    """nbl_create_bp_wide itself, device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in nb.datafiles.gf_tables(code.q))
    prm = nb.binding.Params(method, 5, 4, 2, 1.0, 0.0, 2, 2, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_bp_wide(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def _past_every_check(rc, msg):
    """what an accepted request gives with device -1: no device at all, or an index out of range"""
    return (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg)


def lds_bytes(q, maxdc):
    """the library's own figure: the function both launchers size by"""
    fn = nb.load_library().nbl_debug_bp_wide_lds_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_int32] * 2
    return int(fn(q, maxdc))


def test_header_states_the_limit_and_the_library_exports_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nbldpc.h")).read()
    assert "#define NBL_BP_MAX_CHECK_DEGREE 32" in text and "#define NBL_BP_WIDE_LAYERED 1u" in text
    assert "nbl_create_bp_wide" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_bp_wide")
    assert nb.binding.BP_WIDE_LAYERED == 1


def test_create_bp_wide_degree_limits_come_before_the_device():
    """Both schedules: a check of degree 32 (and of 9) is accepted -- NBL_ERR_NO_DEVICE on a box without a GPU, a decoder on one; degree 33
    is NBL_ERR_ARG and the text names the entry point, 33 and 32, not "(8)"; a variable of degree 9 keeps the text of nbl_create.
    nbl_create and nbl_create_layered_bp still refuse a degree-9 check with their old text."""
    dc32, dc33, dc9, dv9, both = _graphs()
    for code in (dc32, dc9, _ring_code(256, 20, 32), nb.Code(GF16)):
        for layers in (None, "greedy", nb.layer_greedy(code)):
            kw = dict(layers=layers, bp_wide=True, **BP)
            if _no_device():
                _refused(code, -3, "no CPU decode path", **kw)
            else:
                nb.Decoder(code, **kw).close()
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(code), 1)):
            assert _past_every_check(*_create_wide(code, lay, flags)), (lay, flags)
    for layers in (None, "greedy"):
        _refused(dc33, -1, "nbl_create_bp_wide", "check degree 33", "(32)", layers=layers, bp_wide=True, **BP)
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, bp_wide=True, **BP)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, bp_wide=True, **BP)
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(dc33, layers=layers, bp_wide=True, **BP)
        assert "(8)" not in str(e.value)
    for code in (dc9, dc32):
        _refused(code, -1, "node degree above the supported maximum (8)", **BP)
        _refused(code, -1, "node degree above the supported maximum (8)", layers="greedy", bp=True, **BP)


def test_create_bp_wide_refusals_of_method_flags_and_layers():
    dc32 = _graphs()[0]
    for code in (dc32, nb.Code(GF16)):
        for method, extra in ((nb.METHOD_EMS, dict(ems_nm=4, ems_nc=2)), (nb.METHOD_TEMS, {}), (nb.METHOD_BS_TEMS, {}), (nb.METHOD_OSD, {}), (3, {}), (0, {})):
            for layers in (None, "greedy"):
                _refused(code, -2, "nbl_create_bp_wide", "(method 1)", method=method, max_iter=5, layers=layers, bp_wide=True, **extra)
            rc, msg = _create_wide(code, None, 0, method=method)
            assert rc == -2 and "nbl_create_bp_wide" in msg and "(method 1)" in msg, (method, rc, msg)
        for flags in (2, 3, 0x80000000):
            rc, msg = _create_wide(code, None, flags)
            assert rc == -1 and "unknown flag bit" in msg and "NBL_BP_WIDE_LAYERED" in msg, (flags, rc, msg)
        rc, msg = _create_wide(code, nb.layer_greedy(code), 0)
        assert rc == -1 and "nbl_create_bp_wide" in msg and "layer_of = NULL" in msg, (rc, msg)
    # everything else nbl_create refuses, with its text
    _refused(dc32, -1, "max_iter < 0", method=nb.METHOD_BP, max_iter=-1, bp_wide=True)
    _refused(_ring_code(512, 8, 4), -2, "GF(256)", bp_wide=True, gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **BP)
    broken = _ring_code(16, 20, 32)
    broken.chk_h = broken.chk_h.copy()
    broken.chk_h[2] = 0
    _refused(broken, -1, "zero coefficient", bp_wide=True, **BP)
    # the Python class refuses the options the entry point has no argument for, and the other wide kinds beside it
    for kw in (dict(osd_order=0), dict(bs_nm=4), dict(layers="greedy", damped=True), dict(layers="greedy", bp=True), dict(fht=True), dict(wide=True),
               dict(tems_wide=True)):
        with pytest.raises(ValueError):
            nb.Decoder(dc32, bp_wide=True, **BP, **kw)
    for kw in (dict(fht=True), dict(wide=True), dict(tems_wide=True)):
        with pytest.raises(ValueError):
            debug_plan(dc32, nb.METHOD_BP, bp_wide=True, **kw)


def test_every_layer_assignment_error_keeps_the_text_of_nbl_create_layered():
    """The assignment errors of tests/test_layered_bp.py, on the shipped GF(16) code and on a degree-32 graph: status and text are those
    nbl_create_layered_bp gives where it accepts the graph."""
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
            _refused(code, -1, *words, layers=layers, bp_wide=True, **BP)
            rc, msg = _create_wide(code, layers, 1)
            assert rc == -1 and all(w in msg for w in words), (rc, msg)
            if code.chk_deg.max() <= 8:
                with pytest.raises(nb.NblError) as e:
                    nb.Decoder(code, layers=layers, bp=True, **BP)
                assert str(e.value).endswith(msg) or msg in str(e.value), (str(e.value), msg)


def test_lds_size_function_stays_below_the_limit_of_a_workgroup():
    """[maxdc][q] inputs, one [q] vector, two [q] blocks of 16 bytes and 32 reduction words: (maxdc + 5) q 8 + 256 bytes.  The figure
    stays at or below 160 KB for every shape the ABI accepts, so creation refuses no shape for LDS (the degree-32 GF(256) ring code
    above is accepted)."""
    for q in (4, 8, 16, 32, 64, 128, 256):
        for dc in range(2, 33):
            assert lds_bytes(q, dc) == (dc + 5) * q * 8 + 256 <= MAX_LDS, (q, dc)
    assert lds_bytes(256, 32) == 76032 > 64 * 1024 >= lds_bytes(256, 26)   # the launchers opt in above 64 KB: the GF(256) GPU case is above


def test_plan_names_the_wide_kernels():
    """A code with a check above degree 8 -> bp_wide / bp_wide_layered under every debug switch; any other code gets the plan of nbl_create
    / nbl_create_layered_bp, fused kernels included, under switches 0 - 2, and the wide kinds under switch 3 with the same `fusable`."""
    codes = [bc.wide_case(name)[0] for name in bc.NAMES] + [_ring_code(16, 20, 32), _ring_code(256, 20, 32), _graphs()[2]]
    for code in codes:
        assert code.chk_deg.max() > 8
        for fg, rs in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, force_generic=fg, record_state=rs) == ("bp_wide", False, False, True)
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, layers="greedy", force_generic=fg, record_state=rs) == ("bp_wide_layered", False, False, True)
    small = [profile_code("all", q)[0] for q in (4, 8, 16)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4), _ring_code(16, 12, 8),
                                                              _ring_code(128, 8, 4), _ring_code(256, 12, 8)]
    names = set()
    for code in small:
        assert code.chk_deg.max() <= 8
        for fg, rs in ((0, False), (1, False), (2, False), (0, True), (2, True)):
            plain = debug_plan(code, nb.METHOD_BP, force_generic=fg, record_state=rs)
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, force_generic=fg, record_state=rs) == plain
            names.add(plain[0])
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, layers="greedy", force_generic=fg, record_state=rs) == ("bp_layered", False, False, True)
        for rs in (False, True):
            fusable = debug_plan(code, nb.METHOD_BP)[1]
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, force_generic=3, record_state=rs) == ("bp_wide", fusable, False, True)
            assert debug_plan(code, nb.METHOD_BP, bp_wide=True, layers="greedy", force_generic=3, record_state=rs) == ("bp_wide_layered", False, False, True)
        # the switch means nothing to a decoder of nbl_create / nbl_create_layered_bp
        assert debug_plan(code, nb.METHOD_BP, force_generic=3)[0] in ("bp256", "bp64", "bp_small", "bp")
        assert debug_plan(code, nb.METHOD_BP, layers="greedy", force_generic=3)[0] == "bp_layered"
    assert {"bp256", "bp64", "bp_small", "bp"} <= names, names
    assert debug_plan(_ring_code(256, 8, 4), nb.METHOD_BP, bp_wide=True) == ("bp256", True, True, True)      # the (2,4) GF(256) ring code: fused


@pytest.mark.parametrize("name", WIDE_SETS)
def test_wide_fixtures_canonical_matches_reference(oracle, name):
    """The canonical oracle equals the compiled reference on checks of degree 9 .. 32 (GF(256): 5, 8, 9, 16): decisions, return values
    and syndromes of every frame at every recorded iteration count, post / v2c / c2v of the recorded frame within LLR_TOL = 1e-9 of the
    largest magnitude -- what tests/test_oracle_golden.py holds deg_all_gf16_bp to."""
    g, meta = load_golden(name)
    assert meta["profile"]["method"] == 1 and tog.LLR_TOL == 1e-9
    assert meta["chk_degs"] == ([5, 8, 9, 16] if name == "deg_wide_gf256_bp" else [9, 12, 16, 17, 24, 32])
    assert g["syn_ok"].any() and not g["syn_ok"].all() and len(g["state_iters"]) >= 1
    # (method 1 returns nothing for a frame that does not converge, NBLDPC.cpp:776: `ret` is recorded as -1 there and 1 where syn_ok)
    assert np.array_equal(g["ret"] == 1, g["syn_ok"] == 1)
    tog._check_fixture(oracle, g, meta, name, oracle.CANONICAL, False)
    gap = 0.0
    for k, it in enumerate(g["state_iters"]):
        dec = tog._mk_deg(oracle, meta, it, oracle.CANONICAL)
        dec.decode(g["L_ch"][int(g["state_lanes"][0])])
        for a, ref in zip(dec.state(), (g["st_post"][k, 0], g["st_v2c"][k, 0], g["st_c2v"][k, 0])):
            gap = max(gap, float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))))
    print(name, "largest |canonical - reference| / largest magnitude over the recorded state:", gap)


@pytest.mark.parametrize("fixed", [0, 1])
def test_flooding_restatement_equals_the_oracles_own_decoder(oracle, fixed):
    """tests/bp_wide_ref.py is the oracle's flooding decoder written out: the same outputs, flags, counts and state, bit for bit, on the
    ring case (frames that converge at different iterations and never) and on the GF(16) wide case."""
    for name in (bc.RING, "gf16"):
        code, L, iters = bc.wide_case(name)
        assert debug_plan(code, nb.METHOD_BP, bp_wide=True)[0] == "bp_wide"        # (a case the flooding GPU tests compare with)
        ocode, gf = bc.oracle_code(name)
        od = oracle.Decoder(ocode, gf, oracle.BP, iters, oracle.CANONICAL, fixed_iters=fixed)
        seen = set()
        for b in range(L.shape[0]):
            r, out, it = od.decode(L[b])
            post, v2c, c2v = (x.copy() for x in od.state())
            got = bp_wide_ref.decode_flooding(od, gf.mul, L[b], iters, fixed)
            assert (got[1], got[2]) == (r, it) and np.array_equal(got[0], out), (name, b)
            assert np.array_equal(got[3], post) and np.array_equal(got[4], c2v) and np.array_equal(got[5], v2c), (name, b)
            seen.add((r, it))
        assert name != bc.RING or (len(seen) >= 3 and (0, iters) in seen), seen


def test_the_cases_have_the_degrees_they_are_about():
    want = {"gf64": [9, 17, 32], "gf256": [9, 16, 32], "gf128-mix": [2, 3, 4, 8, 9, 10, 31, 32], "gf16": [9, 12, 16, 17, 24, 32],
            "gf4": [9, 12, 16, 17, 24, 32], bc.RING: [16]}
    assert set(want) == set(bc.NAMES)
    for name in bc.NAMES:
        code, L, iters = bc.wide_case(name)
        assert sorted(set(code.chk_deg.tolist())) == want[name] and code.N <= 96 and L.shape[0] <= bc.B_BATCH, name
        assert lds_bytes(code.q, int(code.chk_deg.max())) <= MAX_LDS
    assert sorted(set(bc.wide_case("gf128-mix")[0].var_deg.tolist())) == [1, 2, 3, 8]
    assert lds_bytes(256, 32) > 64 * 1024 and bc.wide_case("gf256")[1].shape[0] == 2 and bc.wide_case("gf256")[2] == 2


@pytest.mark.parametrize("which", bc.SCHEDULES)
@pytest.mark.parametrize("name", bc.NAMES)
def test_every_gpu_case_decides_with_a_margin(oracle, name, which):
    """A condition on the inputs alone: in every case the GPU tests use, under both schedules and in fixed-iteration mode where they use
    it, no DecideLLRVector call of the restatement (a-posteriori, raw and stored v2c, the implicit 0 included) has its two best
    candidates closer than GAP_MIN = 1e-6 -- so decisions, flags and iteration counts cannot hang on the 1e-9 the LLRs agree to.  Every
    state is finite and some check node ran; the ring case has frames that converge at iteration 1 or 2, later, and never."""
    # (the case is one the wide programme runs under this schedule: what the condition is for)
    assert debug_plan(bc.wide_case(name)[0], nb.METHOD_BP, bp_wide=True, layers=None if which == "flooding" else "greedy")[0] == \
        ("bp_wide" if which == "flooding" else "bp_wide_layered")
    refs = {0: bc.wide_reference(name, which)}
    if name == bc.RING:
        refs[1] = bc.wide_reference(name, which, 1)
    for fixed, ref in refs.items():
        for b, r in enumerate(ref):
            print(name, which, "fixed" if fixed else "early", b, "gap", r[6], "converged", r[1], "iters", r[2])
            assert r[6] >= bc.GAP_MIN, (name, which, fixed, b, r[6])
            assert np.all(np.isfinite(r[3])) and np.all(np.isfinite(r[4])) and np.all(np.isfinite(r[5])), b
            assert r[4].any() or (r[2] == 1 and not fixed), b
    if name == bc.RING:
        flags = [(r[1], r[2]) for r in refs[0]]
        assert any(c and i <= 2 for c, i in flags) and any(c and i > 2 for c, i in flags) and (0, 8) in flags, flags
        assert [(r[1], r[2]) for r in refs[1]] == flags and all(np.array_equal(a[0], b[0]) for a, b in zip(refs[0], refs[1]))


def test_harness_switch_is_checked_before_the_device(tmp_path):
    """NBL_BP_WIDE in the host layer (nbldpc_sim): 1 is taken with a method-1 profile under NBL_SCHEDULE unset / flooding / layered-bp
    (on a box without a GPU the run then ends at the missing device, as with NBL_BP_WIDE=0), any other value, another method, another
    schedule and NBL_BP_CHECK=fht beside it are refused with a text of their own."""
    import subprocess
    from nbldpc_amd import hostlib

    def run(method, **env):
        kw = dict(gfq=16, method=method, max_iter=5, parallel=2, crc_len=8, random_msg=1, min_sim_cycle=4, snr_begin=2.0, snr_step=1.0, snr_stop=2.0)
        hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
        r = subprocess.run([hostlib.SIM_BIN], cwd=str(tmp_path), env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
        return r.returncode, r.stdout + r.stderr
    for env in (dict(NBL_BP_WIDE="1"), dict(NBL_BP_WIDE="1", NBL_SCHEDULE="flooding"), dict(NBL_BP_WIDE="1", NBL_SCHEDULE="layered-bp"), dict(NBL_BP_WIDE="0")):
        rc, text = run(nb.METHOD_BP, **env)
        assert "NBL_BP_WIDE" not in text and ((rc != 0 and "no HIP device" in text) if _no_device() else rc == 0), (env, rc, text)
    for method, env, words in ((nb.METHOD_BP, dict(NBL_BP_WIDE="2"), ("NBL_BP_WIDE=2", "unknown value (0, 1)")),
                               (nb.METHOD_BP, dict(NBL_BP_WIDE="1", NBL_BP_CHECK="fht"), ("NBL_BP_WIDE=1 with NBL_BP_CHECK=fht",)),
                               (nb.METHOD_BP, dict(NBL_BP_WIDE="1", NBL_SCHEDULE="layered"), ("NBL_BP_WIDE=1", "(method 1)", "flooding or layered-bp")),
                               (nb.METHOD_EMS, dict(NBL_BP_WIDE="1"), ("NBL_BP_WIDE=1", "(method 1)"))):
        rc, text = run(method, **env)
        assert rc != 0 and all(w in text for w in words), (env, rc, text)
