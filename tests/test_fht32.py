"""Single-precision FHT sum-product decoding (nbl_create_fht32) without a GPU: the refusals and acceptances of the entry point, the
plan, the float32 definition (tests/fht32_ref.py) against an 80-bit brute-force XOR convolution, the noise condition behind the 2^-16
floor, and the conditions on the inputs of every case the GPU tests compare with (tests/test_gpu_fht32.py imports fht32_case() and
fht32_reference() from here, so each reference is computed once per process).

The cases are the shapes of tests/test_fht.py::fht_case with frames of their own: in float32 one rounding of exp / log moves a message
by about 1e-6 of its vector's largest, so a decision is only pinned where its margin is far above that.  Every frame below is the first
of its seed range (3200 on, chosen on the CPU with the two evaluations of the restatement alone: a condition on the inputs, not on any
kernel) that meets test_conditions_on_every_gpu_case under every schedule of its case; `all-16` meets it at 2 iterations and at no
seed of 1800 at 3."""
import ctypes as C
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import fht_ref as fr
import fht32_ref as f32
import pyoracle
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code, _with_extra_edges
from test_fht import fht_case, _layer_of, SCHEDULES
from test_gpu_layered import assignments
from test_layered import GF16, _refused, oracle_edges
from test_layered_bp import CASES, _frames, _bpsk_llr_zero

BP = dict(method=nb.METHOD_BP, max_iter=5)
LN_FLOOR = f32.FLOOR_LOG2 * np.log(2.0)
GAP_FACTOR = 64.0            # smallest decision gap >= 64 x the largest |difference| of the two evaluations near a vector's top
NEAR = 16.0                  # "near the top": within 16 nats of the vector's maximum
TOL_CAP = 2.0 ** -10         # 16 x D32 stays below this: a wrong butterfly or a wrong edge moves w by O(1)
NOISE_MAX = 2.0 ** -19       # largest |v32 - v80| / t: a relative error of 1/8 or less at the floor

# frame seeds per case (frame kinds as in tests/test_layered_bp.py: gf16 BPSK at 1.5 dB; ring: normal, saturating, mixed; else normal)
FRAME_SEEDS = {
    "gf16": (3203, 3259, 3287, 3312, 3357, 3384, 3409, 3201),
    "ring256": (3267, 3200, 3492),
    "ring64": (3263, 3200, 3264),
    "all-4": (3200,),
    "all-8": (3262,),
    "all-16": (3557,),
    "dv48-32": (3205,),
    "rand128": (3287,),
}
ITERS = {"all-16": 2}        # fewer iterations where 3 cannot meet the conditions


@functools.lru_cache(maxsize=None)
def fht32_case(name):
    """(code, L, max_iter) of a named case: the graph of tests/test_fht.py::fht_case(name), one frame per seed of FRAME_SEEDS"""
    code, _, iters = fht_case(name)
    kinds = "b" * 8 if name == "gf16" else "nwm" if name.startswith("ring") else "n"
    rows = []
    for kind, seed in zip(kinds, FRAME_SEEDS[name]):
        rng = np.random.default_rng(seed)
        rows.append(_bpsk_llr_zero(rng, code, 1, 1.5)[0] if kind == "b" else _frames(rng, code.N, code.q, kind)[0])
    return code, np.stack(rows), ITERS.get(name, iters)


@functools.lru_cache(maxsize=None)
def _checks(name):
    code = fht_case(name)[0]
    pyoracle.build()
    ocode, gf = pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q)
    assert np.array_equal(gf.mul, np.array(nb.datafiles.gf_tables(code.q)[0]))
    return f32.Fht32Check(ocode, gf.mul), f32.Fht32Check(ocode, gf.mul, via64=True)


@functools.lru_cache(maxsize=None)
def fht32_reference(name, which, fixed=0, via64=False):
    """[(out, converged, iters, post, c2v, v2c, gap)] per frame of a case under schedule `which` (flooding | greedy | serial | other) in
    float32 (numpy's exp / log, or the second evaluation); computed once and shared"""
    _, L, iters = fht32_case(name)
    return [fr.decode(_checks(name)[int(via64)], L[b], _layer_of(name, which), iters, fixed) for b in range(L.shape[0])]


def tolerance(name, which, fixed=0):
    """the GPU tolerance of a case: 16 x its recorded D32"""
    return 16.0 * f32.D32[(name + "-fixed" if fixed else name, which)]


def _create_fht32(code, layer_of, flags, params=None):
    """nbl_create_fht32 itself at device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in nb.datafiles.gf_tables(code.q))
    prm = params if params is not None else nb.binding.Params(nb.METHOD_BP, 5, 32, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_fht32(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def _device_stage(rc, msg):
    return (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg)


def degree9_code():
    """the shipped GF(16) code with variables joined to check 0 until it has degree 9 (variable degrees stay within 8)"""
    code = nb.Code(GF16)
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    inside = set(code.chk_var[off[0]:off[1]].tolist())
    for n in range(code.N):
        if code.chk_deg[0] >= 9:
            break
        if n not in inside:
            code = _with_extra_edges(code, n, [0])
            inside.add(n)
    assert code.chk_deg.max() == 9 and code.var_deg.max() <= 8
    return code


def test_library_exports_nbl_create_fht32():
    # (not in nb.EXPORTS: tests/test_abi.py holds that list equal to the names its pattern finds in the header, and the pattern stops at a digit)
    assert hasattr(nb.load_library(), "nbl_create_fht32")
    ring = _ring_code(16, 12, 8)                         # the plan query knows the kind by its name, under both schedules
    assert debug_plan(ring, nb.METHOD_BP, fht32=True)[0] == "fht32" and debug_plan(ring, nb.METHOD_BP, fht32=True, layers="greedy")[0] == "fht32_layered"
    assert nb.FHT32_LAYERED == 1 and nb.load_library().nbl_abi_version() == 1


def test_create_fht32_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    # ---- the flags ----
    for flags in (2, 3, 1 << 31):
        rc, msg = _create_fht32(code, None, flags)
        assert rc == -1 and "nbl_create_fht32" in msg and "unknown flag bit" in msg and "NBL_FHT32_LAYERED" in msg, (flags, rc, msg)
    rc, msg = _create_fht32(code, greedy, 0)
    assert rc == -1 and "nbl_create_fht32" in msg and "layer assignment belongs to the layered schedule" in msg, (rc, msg)
    # ---- a valid request reaches the device stage (device -1: it fails there, last) ----
    for lay, flags in ((None, 0), (None, 1), (greedy, 1)):
        assert _device_stage(*_create_fht32(code, lay, flags)), (lay is None, flags)
    # ---- any method but 1: NBL_ERR_UNSUPPORTED, the message names method 1 ----
    for method in (nb.METHOD_EMS, nb.METHOD_TEMS, nb.METHOD_OSD, nb.METHOD_BS_TEMS, 3, 0):
        prm = nb.binding.Params(method, 5, 32, 3, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
        for lay, flags in ((None, 0), (None, 1), (greedy, 1)):
            rc, msg = _create_fht32(code, lay, flags, prm)
            assert rc == -2 and "nbl_create_fht32" in msg and "log-QSPA (method 1) only" in msg, (method, rc, msg)
        _refused(code, -2, "nbl_create_fht32", "log-QSPA (method 1) only", fht32=True, method=method, max_iter=5)
    # ---- a degree-9 check: NBL_ERR_ARG; the message names the entry point, 9 and 8, and points to nbl_create_fht ----
    nine = degree9_code()
    for lay, flags in ((None, 0), (None, 1)):
        rc, msg = _create_fht32(nine, lay, flags)
        assert rc == -1 and "nbl_create_fht32" in msg and "check degree 9 " in msg and "(8)" in msg and "nbl_create_fht " in msg, (rc, msg)
    with pytest.raises(nb.NblError) as e:                # (the same code passes the checks of nbl_create_fht)
        nb.Decoder(nine, fht=True, device=-1, **BP)
    assert _device_stage(e.value.status, str(e.value).split(": ", 1)[1])
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
    _refused(code, -1, "share variable", layers=shared, fht32=True, **BP)
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad_neg, fht32=True, **BP)
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad_gap, fht32=True, **BP)
    _refused(code, -1, "empty layer", layers=bad_big, fht32=True, **BP)
    for lay in (shared, bad_neg, bad_gap, bad_big):      # the same status and text as nbl_create_layered_bp gives
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(code, layers=lay, fht32=True, **BP)
        with pytest.raises(nb.NblError) as f:
            nb.Decoder(code, layers=lay, bp=True, **BP)
        assert (e.value.status, str(e.value)) == (f.value.status, str(f.value))
    # ---- everything else nbl_create refuses, the same way, under both schedules ----
    mul, inv = (np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(16))
    bad_mul = mul.copy()
    bad_mul[3, 5] ^= 1
    broken_h = nb.Code(GF16)
    broken_h.var_h = broken_h.var_h.copy()
    broken_h.var_h[0] ^= 1
    zero_h = nb.Code(GF16)
    zero_h.chk_h = zero_h.chk_h.copy()
    zero_h.chk_h[2] = 0
    dv9 = _with_extra_edges(nb.Code(GF16), 0, [m for m in range(code.M) if m not in code.var_chk[:code.var_deg[0]].tolist()][:9 - int(code.var_deg[0])])
    assert dv9.var_deg.max() == 9
    for layers in (None, "greedy"):
        for c, kw in ((code, dict(method=nb.METHOD_BP, max_iter=-1)),
                      (_ring_code(512, 8, 4), dict(gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **BP)),
                      (broken_h, BP), (zero_h, BP), (code, dict(gf=(bad_mul, inv), **BP)), (dv9, BP)):
            with pytest.raises(nb.NblError) as e:
                nb.Decoder(c, layers=layers, fht32=True, **kw)
            with pytest.raises(nb.NblError) as f:
                nb.Decoder(c, **kw)
            assert f.value.status in (-1, -2) and (e.value.status, str(e.value)) == (f.value.status, str(f.value)), (layers, kw)
    # ---- the Python layer: fht32 goes with layers alone ----
    for kw in (dict(fht=True), dict(bp=True, layers="greedy"), dict(damped=True, layers="greedy"), dict(bp_wide=True), dict(osd_order=0), dict(bs_nm=4)):
        with pytest.raises(ValueError):
            nb.Decoder(code, fht32=True, **kw, **BP)
    for kw in (dict(wide=True), dict(tems_wide=True)):
        with pytest.raises(ValueError):
            nb.Decoder(code, fht32=True, max_iter=5, method=nb.METHOD_BP, **kw)
    with pytest.raises(ValueError):
        debug_plan(code, nb.METHOD_BP, fht=True, fht32=True)


def test_create_fht32_accepts_valid_requests():
    """The checks precede the device: an accepted request fails with NBL_ERR_NO_DEVICE on a box without a GPU and makes a decoder on one.
    The largest shape of the envelope (GF(256), check degree 8: 8 KB of LDS) is accepted."""
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    for c, layers in ((code, None), (code, "greedy"), (code, greedy), (code, np.arange(code.M)), (_ring_code(256, 12, 8), None),
                      (_ring_code(256, 12, 8), "greedy"), (profile_code("all", 256)[0], None), (profile_code("all", 4)[0], "greedy")):
        kw = dict(layers=layers, fht32=True, **BP)
        if _no_device():
            _refused(c, -3, "no CPU decode path", **kw)
        else:
            dec = nb.Decoder(c, **kw)
            want = None if layers is None else nb.layer_greedy(c) if isinstance(layers, str) else np.asarray(layers)
            assert dec.layers is None if want is None else np.array_equal(dec.layers, want)
            dec.close()


def test_plan_names_the_fht32_kernels():
    """(method 1, fht32) -> fht32 / fht32_layered, never fused, v2c kept, on a shipped GF(16), GF(64) and GF(256) code and the `all`
    degree profile, under every force_generic value; the FP64 kind's plan stays"""
    shipped = {}
    for name in sorted(nb.datafiles.codes()):
        c = nb.Code(name)
        if c.chk_deg.max() <= 8:
            shipped.setdefault(c.q, c)
    assert {16, 64, 256} <= set(shipped)
    codes = [shipped[16], shipped[64], shipped[256]] + [profile_code("all", q)[0] for q in (4, 8, 16, 32, 64, 128, 256)]
    for code in codes:
        for fg in (0, 1, 2, 3):
            for rs in (False, True):
                assert debug_plan(code, nb.METHOD_BP, fht32=True, force_generic=fg, record_state=rs) == ("fht32", False, False, True)
                assert debug_plan(code, nb.METHOD_BP, fht32=True, layers="greedy", force_generic=fg, record_state=rs) == ("fht32_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP, fht=True) == ("fht", False, False, True)
        assert debug_plan(code, nb.METHOD_BP, fht=True, layers="greedy") == ("fht_layered", False, False, True)


def _rel(x):
    """LLR rows [n][q-1] -> log-probabilities relative to the vector's largest, [n][q], the implicit 0 of slot 0 included"""
    full = np.concatenate([np.zeros(x.shape[:-1] + (1,), dtype=x.dtype), x], axis=-1)
    return full - full.max(axis=-1, keepdims=True)


@pytest.mark.parametrize("q", [4, 16, 256])
@pytest.mark.parametrize("dc", [2, 4, 8])
def test_check_node32_equals_the_brute_force_convolution(q, dc):
    """The float32 restatement's c2v against the exact box-plus (direct XOR convolution, 80-bit) of the same float32 inputs, 20 checks
    each: every entry whose exact probability is above 2^-12 of its vector's largest agrees within a relative 2^-6 (the transform's
    noise is about 2^-21 of the largest, 2^-9 of such an entry), and no output lies below -16 ln 2 of its vector's maximum, to float32
    rounding: log v reaches 56 ln 2 = 38.8 (ulp 3.8e-6), and two logs within 2 ulp and two subtractions make 5 ulp, 2e-5."""
    rng = np.random.default_rng(3200 + 1000 * q + dc)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    worst, compared = 0.0, 0
    for _ in range(20):
        vin = rng.normal(-2, 4, (dc, q - 1)).astype(np.float32)
        h = rng.integers(1, q, dc)
        got = f32.check_node32(vin, h, mul)
        assert got.dtype == np.float32 and np.all(np.isfinite(got))
        exact = _rel(fr.brute_force(vin, h, mul))
        mine = _rel(got.astype(np.longdouble))
        above = exact > -12 * np.log(2.0)
        worst = max(worst, float(np.max(np.abs(np.expm1(mine - exact))[above])))
        compared += int(above.sum())
        assert float(mine.min()) >= -LN_FLOOR - 2e-5, float(mine.min())
    print(q, dc, "largest relative error above 2^-12:", worst, "= 2^%.1f" % np.log2(max(worst, 1e-300)), "over", compared, "entries")
    assert compared >= 20 * dc and worst <= 2.0 ** -6


def test_one_hot_inputs_give_finite_outputs_at_the_floor():
    """normal(-900, 700) inputs: every vector one-hot after step 2, but for the rare one whose two largest entries lie within a few
    nats.  The outputs are finite, none lies below -16 ln 2 of its vector's largest (to the rounding of a float32 log), and more than
    nine in ten sit at that floor."""
    q, dc = 64, 4
    rng = np.random.default_rng(3264)
    mul = np.array(nb.datafiles.gf_tables(q)[0])
    for _ in range(5):
        vin, h = rng.normal(-900, 700, (dc, q - 1)).astype(np.float32), rng.integers(1, q, dc)
        for via64 in (False, True):
            got = f32.check_node32(vin, h, mul, via64)
            assert np.all(np.isfinite(got))
            rel = np.sort(_rel(got.astype(np.float64)), axis=1)
            assert np.all(rel[:, -1] == 0.0) and rel.min() >= -LN_FLOOR - 4e-6, rel[:, :3]
            assert (np.abs(rel + LN_FLOOR) <= 4e-6).mean() > 0.9, rel[:, -4:]


def test_degree_two_returns_the_partner_re_permuted():
    """dc = 2: each output is WHT(WHT(u)) / q = u of the other edge, to rounding.  An entry r nats below its vector's largest comes back
    with a relative error of about q 2^-24 e^r: inputs uniform in (-1.5, 1.5) are 3 nats wide, so at q = 256 an entry and the slot-0
    entry it is measured from are each within 256 x 2^-24 x e^3 = 3.1e-4, their difference within 1e-3."""
    for q in (4, 16, 256):
        rng = np.random.default_rng(3200 + q)
        mul = np.array(nb.datafiles.gf_tables(q)[0])
        inv = np.array(nb.datafiles.gf_tables(q)[1])
        vin, h = rng.uniform(-1.5, 1.5, (2, q - 1)).astype(np.float32), rng.integers(1, q, 2)
        got = f32.check_node32(vin, h, mul)
        for d in (0, 1):
            o = 1 - d
            full = np.concatenate([[0.0], vin[o].astype(np.float64)])
            want = np.array([full[mul[inv[h[o]], mul[h[d], a]]] for a in range(1, q)])   # c2v_d[a] = in_o[h_o^-1 h_d a]
            assert np.max(np.abs(got[d] - want)) <= 1e-3, (q, d)


def test_layered_restatement_with_one_layer_per_check():
    """the float32 layered restatement with one layer per check in check order (the `serial` assignment of the GPU tests) equals the
    same function called with that assignment written out, and every array it returns is float32"""
    code, L, iters = fht32_case("ring64")
    chk = _checks("ring64")[0]
    serial = assignments(code)["serial"]
    explicit = [m for m in range(code.M)]
    for b in range(L.shape[0]):
        a, x = fr.decode_layered(chk, L[b], serial, iters), fr.decode_layered(chk, L[b], explicit, iters)
        assert (a[1], a[2], a[6]) == (x[1], x[2], x[6])
        for k in (0, 3, 4, 5):
            assert np.array_equal(a[k], x[k]), (b, k)
        assert all(a[k].dtype == np.float32 for k in (3, 4, 5))


GPU_CASES = [(name, which, 0) for name, _ in CASES for which in SCHEDULES[name]] + [("gf16", "flooding", 1), ("gf16", "greedy", 1)]
GPU_IDS = [f"{n}-{w}{'-fixed' if f else ''}" for n, w, f in GPU_CASES]


def _near_top_difference(a, x):
    """largest |a - x| over post / v2c entries within NEAR of their vector's maximum"""
    worst = 0.0
    for k in (3, 5):
        p, r = np.asarray(a[k], dtype=np.float64), np.asarray(x[k], dtype=np.float64)
        near = (_rel(p) >= -NEAR)[:, 1:]
        worst = max(worst, float(np.max(np.abs(p - r)[near])) if near.any() else 0.0)
    return worst


@pytest.mark.parametrize("name,which,fixed", GPU_CASES, ids=GPU_IDS)
def test_conditions_on_every_gpu_case(oracle, name, which, fixed):
    """Conditions on the inputs alone, for every case tests/test_gpu_fht32.py uses: (a) the two evaluations of the restatement (numpy's
    float32 exp / log; exp / log in float64 rounded once) give the same out_sym, flags and iteration counts; (b) the smallest decision
    gap is at least 64 x the largest absolute difference between the two over post / v2c entries within 16 of their vector's maximum;
    (c) D32, their largest deviation in the probability domain, equals the recorded value (to 5 %: two numpy builds may round an exp
    differently); (d) 16 x D32 <= 2^-10."""
    ra, rb = fht32_reference(name, which, fixed), fht32_reference(name, which, fixed, True)
    d32 = 0.0
    for b, (a, x) in enumerate(zip(ra, rb)):
        d, diff, gap = fr.state_dev(a, x), _near_top_difference(a, x), min(a[6], x[6])
        print(name, which, fixed, b, "gap", gap, "difference near the top", diff, "converged", a[1], "iters", a[2], "D32", d)
        assert np.array_equal(a[0], x[0]) and (a[1], a[2]) == (x[1], x[2]), b
        assert all(np.all(np.isfinite(a[k])) and a[k].dtype == np.float32 for k in (3, 4, 5)) and (np.any(a[4] != 0.0) or a[2] == 1), b
        assert gap >= GAP_FACTOR * diff and gap >= 1e-6, (b, gap, diff)
        d32 = max(d32, d)
    rec = f32.D32[(name + "-fixed" if fixed else name, which)]
    print(name, which, fixed, "D32", d32, "recorded", rec, "tolerance", 16 * rec)
    assert 16.0 * d32 <= TOL_CAP and 16.0 * rec <= TOL_CAP
    assert abs(d32 - rec) <= 0.05 * rec, (d32, rec)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_transform_noise_stays_below_the_floor(oracle, name):
    """On every check of every GPU case, fed the v2c vectors the flooding restatement gives it in every iteration: the largest
    |v32 - v80| / t over the check's outputs is at most 2^-19, which keeps the relative error of an entry at the 2^-16 floor at 1/8 or
    less (measured when the floor was chosen: 2^-20.7 at worst, q = 256 and degree 8)."""
    code, L, iters = fht32_case(name)
    chk = _checks(name)[0]
    worst = [0.0]

    class Probe(f32.Fht32Check):
        def check(self, m, vin):
            g = self.g
            worst[0] = max(worst[0], f32.noise_over_t(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul))
            return super().check(m, vin)

    probe = Probe(chk.code, chk.mul)
    for b in range(L.shape[0]):
        fr.decode_flooding(probe, L[b], iters)
    print(name, "largest |v32 - v80| / t = 2^%.2f" % np.log2(worst[0]))
    assert 0.0 < worst[0] <= NOISE_MAX


def test_gf16_frames_converge_at_different_iterations_and_never(oracle):
    for which in ("flooding", "greedy"):
        flags = [(r[1], r[2]) for r in fht32_reference("gf16", which)]
        assert len({i for c, i in flags if c}) >= 2 and any(not c for c, _ in flags), (which, flags)
    # the saturating frames of the ring cases do saturate: most c2v entries sit at the floor
    for name in ("ring64", "ring256"):
        c2v = fht32_reference(name, "flooding")[1][4].astype(np.float64)
        at_floor = np.abs(_rel(c2v) + LN_FLOOR) < 1e-5
        assert at_floor.mean() > 0.9, (name, at_floor.mean())
