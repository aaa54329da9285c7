"""FHT sum-product decoding (nbl_create_fht) without a GPU: the refusals and acceptances of the entry point, the plan, the definition
(tests/fht_ref.py) against an 80-bit brute-force XOR convolution, and the conditions on the inputs of every case the GPU tests compare
with (tests/test_gpu_fht.py imports fht_case() and fht_reference() from here, so each reference is computed once per process)."""
import ctypes as C
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import fht_ref as fr
import layered_bp_ref as lbr
import pyoracle
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_gpu_layered import assignments
from test_layered import GF16, _refused, oracle_edges
from test_layered_bp import CASES, _frames, case

BP = dict(method=nb.METHOD_BP, max_iter=5)
GAP_MIN = 1e-6       # (a) smallest decide gap a case may have
D80_MAX = 1e-10      # (c) largest probability-domain deviation between the FP64 and the 80-bit restatement
LN_FLOOR = fr.FLOOR_LOG2 * np.log(2.0)

# Inputs of our own where those of tests/test_layered_bp.py do not meet (c): the mixed frame of `ring256` drifts to 8.7e-8 under the
# greedy assignment.  2566 is the first seed from 2560 on at which every schedule of the case stays below 1e-11 (chosen on the CPU with
# the restatement alone; a condition on the inputs, not on any kernel).
OWN_SEEDS = {"ring256": 2566}
SCHEDULES = {name: ("flooding",) + whiches for name, whiches in CASES}


@functools.lru_cache(maxsize=None)
def fht_case(name):
    """(code, L, max_iter) of a named case: the shapes of tests/test_layered_bp.py::case, inputs of our own where OWN_SEEDS says so"""
    code, L, iters = case(name)
    if name in OWN_SEEDS:
        L = _frames(np.random.default_rng(OWN_SEEDS[name]), code.N, code.q, "nwm")
    return code, L, iters


@functools.lru_cache(maxsize=None)
def _checks(name):
    code = fht_case(name)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    return fr.FhtCheck(ocode, gf.mul), fr.FhtCheck(ocode, gf.mul, np.longdouble)


def _layer_of(name, which):
    return None if which == "flooding" else assignments(fht_case(name)[0])[which]


@functools.lru_cache(maxsize=None)
def fht_reference(name, which, fixed=0):
    """[(out, converged, iters, post, c2v, v2c, gap)] per frame of a case under schedule `which` (flooding | greedy | serial | other) in
    FP64; computed once and shared"""
    _, L, iters = fht_case(name)
    return [fr.decode(_checks(name)[0], L[b], _layer_of(name, which), iters, fixed) for b in range(L.shape[0])]


@functools.lru_cache(maxsize=None)
def fht_reference80(name, which, fixed=0):
    _, L, iters = fht_case(name)
    return [fr.decode(_checks(name)[1], L[b], _layer_of(name, which), iters, fixed) for b in range(L.shape[0])]


def tolerance(name, which, fixed=0):
    """the GPU tolerance of a case: 16 x its recorded D80"""
    return 16.0 * fr.D80[(name + "-fixed" if fixed else name, which)]


def _create_fht(code, layer_of, flags, params=None, gf=None):
    """nbl_create_fht itself (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = gf if gf is not None else (np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(code.q))
    mul, inv = np.ascontiguousarray(mul), np.ascontiguousarray(inv)
    prm = params if params is not None else nb.binding.Params(nb.METHOD_BP, 5, 32, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_fht(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def test_library_exports_nbl_create_fht():
    assert "nbl_create_fht" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_fht")
    assert nb.load_library().nbl_abi_version() == 1


def test_create_fht_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    # ---- the flags ----
    for flags in (2, 3, 1 << 31):
        rc, msg = _create_fht(code, None, flags)
        assert rc == -1 and "unknown flag bit" in msg and "NBL_FHT_LAYERED" in msg, (flags, rc, msg)
    rc, msg = _create_fht(code, greedy, 0)
    assert rc == -1 and "layer assignment belongs to the layered schedule" in msg, (rc, msg)
    # (device -1: an accepted request fails on the device, last)
    for lay, flags in ((None, 0), (None, 1), (greedy, 1)):
        rc, msg = _create_fht(code, lay, flags)
        assert (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg), (rc, msg)
    # ---- any method but 1: the message names method 1 ----
    for method in (nb.METHOD_EMS, nb.METHOD_TEMS, nb.METHOD_OSD, nb.METHOD_BS_TEMS, 3, 0):
        for layers in (None, "greedy", greedy):
            _refused(code, -2, "nbl_create_fht", "log-QSPA (method 1) only", layers=layers, fht=True, method=method, max_iter=5)
    # ---- every assignment error of nbl_create_layered, with its status and text ----
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    v = int(code.chk_var[0])
    other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
    shared = greedy.copy()
    shared[other] = shared[0]
    first = next((m, int(x)) for m in range(code.M) for x in code.chk_var[off[m]:off[m + 1]]
                 if any(shared[k] == shared[m] and int(x) in code.chk_var[off[k]:off[k + 1]].tolist() for k in range(m)))
    partner = next(k for k in range(first[0]) if shared[k] == shared[first[0]] and first[1] in code.chk_var[off[k]:off[k + 1]].tolist())
    _refused(code, -1, f"checks {partner} and {first[0]} ", f"share variable {first[1]}", layers=shared, fht=True, **BP)
    bad = greedy.copy()
    bad[3] = -1
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad, fht=True, **BP)
    bad = greedy.copy()
    bad[bad == bad.max()] += 1
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad, fht=True, **BP)
    bad = greedy.copy()
    bad[5] = 1 << 30
    _refused(code, -1, "empty layer", layers=bad, fht=True, **BP)
    for lay in (shared, bad):                            # the same status and text as nbl_create_layered_bp gives
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(code, layers=lay, fht=True, **BP)
        with pytest.raises(nb.NblError) as f:
            nb.Decoder(code, layers=lay, bp=True, **BP)
        assert (e.value.status, str(e.value)) == (f.value.status, str(f.value))
    # ---- everything nbl_create refuses, the same way, under both schedules ----
    mul, inv = (np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(16))
    bad_mul = mul.copy()
    bad_mul[3, 5] ^= 1
    broken_h = nb.Code(GF16)
    broken_h.var_h = broken_h.var_h.copy()
    broken_h.var_h[0] ^= 1
    zero_h = nb.Code(GF16)
    zero_h.chk_h = zero_h.chk_h.copy()
    zero_h.chk_h[2] = 0
    for layers in (None, "greedy"):
        for c, kw in ((code, dict(method=nb.METHOD_BP, max_iter=-1)),
                      (_ring_code(512, 8, 4), dict(gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **BP)),
                      (broken_h, BP), (zero_h, BP), (code, dict(gf=(bad_mul, inv), **BP))):
            with pytest.raises(nb.NblError) as e:
                nb.Decoder(c, layers=layers, fht=True, **kw)
            with pytest.raises(nb.NblError) as f:
                nb.Decoder(c, **kw)
            assert f.value.status in (-1, -2) and (e.value.status, str(e.value)) == (f.value.status, str(f.value)), (layers, kw)
    # ---- the Python layer: fht goes with layers alone ----
    for kw in (dict(bp=True, layers="greedy"), dict(damped=True, layers="greedy"), dict(osd_order=0), dict(bs_nm=4)):
        with pytest.raises(ValueError):
            nb.Decoder(code, fht=True, **kw, **BP)


def test_create_fht_accepts_valid_requests():
    """The checks of nbl_create_fht precede the device: an accepted request fails with NBL_ERR_NO_DEVICE on a box without a GPU and
    makes a decoder on one.  The largest shape of the envelope (GF(256), check degree 8: 16 KB of LDS) is accepted."""
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    for c, layers in ((code, None), (code, "greedy"), (code, greedy), (code, np.arange(code.M)), (_ring_code(256, 12, 8), None),
                      (_ring_code(256, 12, 8), "greedy"), (profile_code("all", 256)[0], None), (profile_code("all", 4)[0], "greedy")):
        kw = dict(layers=layers, fht=True, **BP)
        if _no_device():
            _refused(c, -3, "no CPU decode path", **kw)
        else:
            dec = nb.Decoder(c, **kw)
            want = None if layers is None else nb.layer_greedy(c) if isinstance(layers, str) else np.asarray(layers)
            assert dec.layers is None if want is None else np.array_equal(dec.layers, want)
            dec.close()


def test_plan_names_the_fht_kernels():
    """(method 1, fht) -> fht / fht_layered over q = 4 .. 256, never fused, v2c kept, in every variant; every other plan stays"""
    codes = [profile_code("all", q)[0] for q in (4, 8, 16, 32, 64, 128, 256)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4)]
    for code in codes:
        for fg, rs in ((0, False), (1, False), (2, False), (0, True)):
            assert debug_plan(code, nb.METHOD_BP, fht=True, force_generic=fg, record_state=rs) == ("fht", False, False, True)
            assert debug_plan(code, nb.METHOD_BP, fht=True, layers="greedy", force_generic=fg, record_state=rs) == ("fht_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP, layers="greedy") == ("bp_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP)[0] in ("bp256", "bp64", "bp_small", "bp")
        assert debug_plan(code, nb.METHOD_BP, force_generic=1)[0] == "bp"


def _bpsk_vectors(rng, q, dc, ebn0_db=2.0):
    p = q.bit_length() - 1
    sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * rng.standard_normal((dc, p))) / sigma ** 2
    a = np.arange(1, q)
    return bit @ ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64).T


@pytest.mark.parametrize("q,dc,kind,tol", [(16, 4, "normal", 1e-9), (64, 5, "normal", 1e-9), (256, 4, "normal", 1e-9), (256, 8, "normal", 1e-9),
                                           (256, 4, "bpsk", 1e-5), (256, 8, "bpsk", 1e-5)])
def test_check_node_equals_the_brute_force_convolution(q, dc, kind, tol):
    """The FP64 restatement's c2v against the exact box-plus (direct XOR convolution, 80-bit): every entry more than one nat above the
    floor agrees to `tol` (the prototype measured 1e-12 / 8e-7), and every vector decides the same.  20 checks each.  A property of the
    definition, not of a kernel."""
    rng = np.random.default_rng(1000 * q + dc)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    worst, compared = 0.0, 0
    for _ in range(20):
        vin = rng.normal(-2, 4, (dc, q - 1)) if kind == "normal" else _bpsk_vectors(rng, q, dc)
        h = rng.integers(1, q, dc)
        got, exact = fr.check_node(vin, h, mul), fr.brute_force(vin, h, mul)
        above = exact > np.maximum(exact.max(axis=1, keepdims=True), 0.0) - LN_FLOOR + 1.0
        worst = max(worst, float(np.max(np.abs(got - exact)[above])))
        compared += int(above.sum())
        for d in range(dc):
            assert lbr._decide(got[d]) == lbr._decide(np.asarray(exact[d], dtype=np.float64)), d
        assert np.all(got >= np.maximum(got.max(axis=1, keepdims=True), 0.0) - LN_FLOOR - 1e-9)   # nothing below the floor
    print(q, dc, kind, "largest |c2v - exact| above the floor:", worst, "over", compared, "entries")
    assert compared > 20 * dc and worst <= tol


def test_degree_two_returns_the_other_edge_re_permuted():
    """dc = 2: V_0 = U_1, V_1 = U_0, so each output is WHT(WHT(u)) / q = u of the other edge, to rounding.  An entry r nats below its
    vector's largest comes back with a relative error of about q 2^-53 e^r (the transform's rounding is relative to the largest), so
    the 1e-12 of the statement is a statement about entries within ln(1e-12 / (256 x 2^-53)) = 3.6 nats: the inputs are uniform in
    (-1.5, 1.5), 3 nats wide with the 0 of slot 0 inside."""
    for q in (4, 16, 256):
        rng = np.random.default_rng(q)
        mul = np.array(nb.datafiles.gf_tables(q)[0])
        inv = np.array(nb.datafiles.gf_tables(q)[1])
        vin, h = rng.uniform(-1.5, 1.5, (2, q - 1)), rng.integers(1, q, 2)
        got = fr.check_node(vin, h, mul)
        for d in (0, 1):
            o = 1 - d
            full = np.concatenate([[0.0], vin[o]])
            want = np.array([full[mul[inv[h[o]], mul[h[d], a]]] for a in range(1, q)])   # c2v_d[a] = in_o[h_o^-1 h_d a]
            assert np.max(np.abs(got[d] - want)) <= 1e-12, (q, d)


def test_one_hot_input_saturates_its_partners_at_the_floor():
    """One input a thousand nats wide (one-hot after step 2): every other output has its largest entry and q - 1 entries at exactly
    -40 ln 2 below it."""
    q, dc = 64, 4
    rng = np.random.default_rng(64)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    vin, h = rng.normal(-2, 4, (dc, q - 1)), rng.integers(1, q, dc)
    for d in range(1, dc):
        vin[d] = -2000.0 - 100.0 * rng.random(q - 1)     # symbol 0, certainly
    vin[0] = -2000.0
    vin[0, 6] = 900.0                                    # symbol 7, certainly
    got = fr.check_node(vin, h, mul)
    for d in range(dc):
        full = np.concatenate([[0.0], got[d]])
        rel = np.sort(full - full.max())
        assert rel[-1] == 0.0 and np.max(np.abs(rel[:-1] + LN_FLOOR)) <= 1e-12, (d, rel[:3], rel[-2:])


def test_layered_restatement_equals_layered_bp_ref_on_the_fht_check():
    """fht_ref.decode_layered in FP64 is layered_bp_ref.decode with FhtCheck as its decoder object, bit for bit"""
    code, L, iters = fht_case("gf16")
    chk = _checks("gf16")[0]
    lay = assignments(code)["greedy"]
    for b in (3, 6):
        mine = fr.decode_layered(chk, L[b], lay, iters)
        theirs = lbr.decode(chk, chk.mul, L[b], lay, iters)
        assert (mine[1], mine[2], mine[6]) == (theirs[1], theirs[2], theirs[8])
        for k in (0, 3, 4, 5):
            assert np.array_equal(mine[k], theirs[k]), (b, k)


GPU_CASES = [(name, which, 0) for name, _ in CASES for which in SCHEDULES[name]] + [("gf16", "flooding", 1), ("gf16", "greedy", 1)]


@pytest.mark.parametrize("name,which,fixed", GPU_CASES, ids=[f"{n}-{w}{'-fixed' if f else ''}" for n, w, f in GPU_CASES])
def test_conditions_on_every_gpu_case(oracle, name, which, fixed):
    """A condition on the inputs alone, for every case tests/test_gpu_fht.py uses: (a) the smallest decide gap is at least 1e-6, (b)
    the FP64 and the 80-bit restatement give the same out, converged and iters, (c) their states differ by at most 1e-10 in the
    probability domain.  The figure of (c) is the one recorded in fht_ref.D80, which the GPU tolerance is 16 times."""
    r64, r80 = fht_reference(name, which, fixed), fht_reference80(name, which, fixed)
    d80 = 0.0
    for b, (a, x) in enumerate(zip(r64, r80)):
        d = fr.state_dev(a, x)
        print(name, which, fixed, b, "gap", a[6], "converged", a[1], "iters", a[2], "D80", d)
        assert min(a[6], x[6]) >= GAP_MIN, (b, a[6], x[6])
        assert np.array_equal(a[0], x[0]) and (a[1], a[2]) == (x[1], x[2]), b
        assert all(np.all(np.isfinite(a[k])) for k in (3, 4, 5)) and (np.any(a[4] != 0.0) or a[2] == 1), b
        d80 = max(d80, d)
    rec = fr.D80[(name + "-fixed" if fixed else name, which)]
    print(name, which, fixed, "D80", d80, "recorded", rec)
    assert d80 <= D80_MAX and rec <= D80_MAX
    assert abs(d80 - rec) <= 0.05 * rec, (d80, rec)


def test_gf16_frames_converge_at_different_iterations_and_never(oracle):
    for which in ("flooding", "greedy"):
        flags = [(r[1], r[2]) for r in fht_reference("gf16", which)]
        assert len({i for c, i in flags if c}) >= 2 and any(not c for c, _ in flags), (which, flags)
    # the saturating frames of the ring cases do saturate: most c2v entries sit at the floor
    for name in ("ring64", "ring256"):
        c2v = fht_reference(name, "flooding")[1][4]
        full = np.concatenate([np.zeros((c2v.shape[0], 1)), c2v], axis=1)
        at_floor = np.abs(full - full.max(axis=1, keepdims=True) + LN_FLOOR) < 1e-9
        assert at_floor.mean() > 0.9, (name, at_floor.mean())
