"""T-EMS decoding on codes whose trellis path does not fit nbl_create's 32-bit code (nbl_create_tems_wide, check degrees 2 .. 32 over any
field) without a GPU: the path code of nbl_tems_path.h against dense digit tuples; the limits of the entry point, all before the device;
the plan; the LDS figure; the oracle pinned to the compiled reference at these degrees (the deg_wide_*_tems fixtures of
tests/golden/make_golden_tems_wide.py); the conditions on the inputs of every case tests/test_gpu_tems_wide.py compares with
(tests/tems_wide_cases.py); and that the integer-valued frames of its ties test discriminate the rule for equal costs."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import tems_wide_cases as tc
import tems_wide_ref
import test_oracle_golden as tog
from conftest import load_golden
from degree_util import TEMS_REFUSED, profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_fht_wide import _graphs
from test_layered import GF16, _refused

TEMS = dict(method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=2)
WIDE_SETS = ["deg_wide_gf64_tems", "deg_wide_gf16_tems", "deg_wide_gf256_tems"]
MAX_LDS = 160 * 1024
MAX_NC = 4


def _create_wide(code, layer_of, flags, tems_nr=2, tems_nc=2, method=nb.METHOD_TEMS):
    """nbl_create_tems_wide itself, device -1 (the Decoder class cannot form every refused request): (status, message)"""
    lib = nb.load_library()
    mul, inv = (np.ascontiguousarray(np.array(t, dtype=np.uint16)) for t in nb.datafiles.gf_tables(code.q))
    prm = nb.binding.Params(method, 5, 4, 2, 1.0, 0.0, tems_nr, tems_nc, 1.0, 0.0, 0, 0, 0)
    desc, h = code.desc(), C.c_void_p()
    lay = None if layer_of is None else np.ascontiguousarray(layer_of, dtype=np.int32)
    rc = lib.nbl_create_tems_wide(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None if lay is None else lay.ctypes.data, flags, -1, C.byref(h))
    assert rc != 0 and not h.value
    return rc, lib.nbl_last_error(None).decode()


def _past_every_check(rc, msg):
    """what an accepted request gives with device -1: no device at all, or an index out of range"""
    return (rc, msg) == (-3, "no HIP device (this library has no CPU decode path)") if _no_device() else (rc == -1 and "device index out of range" in msg)


def lds_bytes(q, maxdc, nr, nc):
    """the library's own figure: the function creation's refusal and both launchers use"""
    fn = nb.load_library().nbl_debug_tems_wide_lds_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_int32] * 4
    return int(fn(q, maxdc, nr, nc))


def path_key(devs):
    """the library's path code of the path that deviates to sym in column col for (col, sym) in devs (columns ascending)"""
    fn = nb.load_library().nbl_debug_tems_wide_path_key
    fn.restype, fn.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p, C.c_int32]
    cols, syms = np.array([d[0] for d in devs], dtype=np.int32), np.array([d[1] for d in devs], dtype=np.int32)
    return int(fn(cols.ctypes.data, syms.ctypes.data, len(devs)))


def path_digit(code, col):
    fn = nb.load_library().nbl_debug_tems_wide_path_digit
    fn.restype, fn.argtypes = C.c_int32, [C.c_uint64, C.c_int32]
    return int(fn(code, col))


def dense(devs, dc):
    t = [0] * dc
    for col, sym in devs:
        t[col] = sym
    return tuple(t)


def test_header_states_the_limit_and_the_library_exports_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nbldpc.h")).read()
    assert "#define NBL_TEMS_MAX_CHECK_DEGREE 32" in text and "#define NBL_TEMS_WIDE_LAYERED 1u" in text
    assert "nbl_create_tems_wide" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_tems_wide")
    assert "#define NBL_TEMS_WIDE_MAX_NC 4" in open(os.path.join(root, "nbldpc_amd", "csrc", "nbl_tems_path.h")).read()
    assert "nbl_tems_path.h" in open(os.path.join(root, "nbldpc_amd", "csrc", "nbl_cn_tems_wide_core.h")).read()     # the programme uses it


def test_path_key_orders_like_the_digit_string_exhaustive():
    """dc 4, q 4, at most 3 deviations: every pair of paths.  Unsigned order and equality of the codes = lexicographic order and equality
    of the dense digit tuples (column 0 most significant); every digit is read back."""
    dc, q = 4, 4
    paths = [tuple(zip(cols, syms)) for n in range(4) for cols in itertools.combinations(range(dc), n) for syms in itertools.product(range(1, q), repeat=n)]
    assert len(paths) == 1 + 4 * 3 + 6 * 9 + 4 * 27
    keys = [path_key(p) for p in paths]
    tuples = [dense(p, dc) for p in paths]
    assert len(set(keys)) == len(paths) and keys[0] == 0
    for p, k in zip(paths, keys):
        assert tuple(path_digit(k, c) for c in range(dc)) == dense(p, dc) and k < 1 << 52
    order_k = sorted(range(len(paths)), key=lambda i: keys[i])
    order_t = sorted(range(len(paths)), key=lambda i: tuples[i])
    assert order_k == order_t                                            # a total order: one comparison of the two sortings covers every pair


def test_path_key_orders_like_the_digit_string_random():
    """dc 32, q 256, up to 4 deviations, columns clustered and spread, small and large symbols: 20,000 random pairs, 0 mismatches of order
    or equality; the digits of all 32 columns are read back."""
    rng = np.random.default_rng(2024)

    def draw():
        n = int(rng.integers(0, MAX_NC + 1))
        lo = int(rng.integers(0, 32))
        pool = np.arange(32) if rng.random() < 0.5 else np.arange(lo, min(32, lo + 5))
        cols = sorted(rng.choice(pool, size=min(n, len(pool)), replace=False).tolist())
        syms = [int(rng.choice([1, 2, 254, 255])) if rng.random() < 0.5 else int(rng.integers(1, 256)) for _ in cols]
        return tuple(zip(cols, syms))
    bad = 0
    for i in range(20000):
        a = draw()
        b = a if i % 50 == 0 else (a[:-1] + ((a[-1][0], 1 + a[-1][1] % 255),) if a and i % 7 == 0 else draw())
        ka, kb, ta, tb = path_key(a), path_key(b), dense(a, 32), dense(b, 32)
        bad += (ka < kb) != (ta < tb) or (ka == kb) != (ta == tb)
        if i % 100 == 0:
            assert tuple(path_digit(ka, c) for c in range(32)) == ta
    assert bad == 0
    # the slot layout the header states: slot 0 at bit 39, slot 3 at bit 0, 13 bits each
    assert path_key([(31, 1)]) == 1 << 39 and path_key([(0, 255)]) == ((31 << 8) | 255) << 39
    assert path_key([(0, 1), (1, 1), (2, 1), (31, 9)]) == (((31 << 8) | 1) << 39) | (((30 << 8) | 1) << 26) | (((29 << 8) | 1) << 13) | 9
    assert path_key([(3, 7), (3, 9)]) == 0 and path_key([(0, 1)] * 5) == 0                     # outside the export's domain


def test_create_tems_wide_degree_limits_come_before_the_device():
    """Both schedules: a check of degree 32 (and of 9) is accepted -- NBL_ERR_NO_DEVICE on a box without a GPU, a decoder on one; so is
    every cell nbl_create refuses for its 32-bit path code; degree 33 is NBL_ERR_ARG and the text names the entry point, 33 and 32, not
    "(8)"; a variable of degree 9 keeps the text of nbl_create."""
    dc32, dc33, dc9, dv9, both = _graphs()
    cells = [profile_code(prof, q)[0] for prof, q in TEMS_REFUSED]
    for code in [dc32, dc9] + cells:
        for layers in (None, "greedy", nb.layer_greedy(code)):
            kw = dict(layers=layers, tems_wide=True, **TEMS)
            if _no_device():
                _refused(code, -3, "no CPU decode path", **kw)
            else:
                nb.Decoder(code, **kw).close()
        for lay, flags in ((None, 0), (None, 1), (nb.layer_greedy(code), 1)):
            assert _past_every_check(*_create_wide(code, lay, flags)), (lay, flags)
    for code in cells:                                                   # nbl_create and nbl_create_layered_ex keep their refusal
        _refused(code, -2, "32-bit", **TEMS)
        _refused(code, -2, "32-bit", layers="greedy", damped=True, **TEMS)
    for layers in (None, "greedy"):
        _refused(dc33, -1, "nbl_create_tems_wide", "check degree 33", "(32)", layers=layers, tems_wide=True, **TEMS)
        _refused(dv9, -1, "node degree above the supported maximum (8)", layers=layers, tems_wide=True, **TEMS)
        _refused(both, -1, "node degree above the supported maximum (8)", layers=layers, tems_wide=True, **TEMS)
        with pytest.raises(nb.NblError) as e:
            nb.Decoder(dc33, layers=layers, tems_wide=True, **TEMS)
        assert "(8)" not in str(e.value)


def test_create_tems_wide_refusals_of_method_flags_layers_and_nc():
    dc32 = _graphs()[0]
    for code in (dc32, nb.Code(GF16)):
        for method, extra in ((nb.METHOD_BP, {}), (nb.METHOD_EMS, dict(ems_nm=4, ems_nc=2)), (nb.METHOD_BS_TEMS, {}), (nb.METHOD_OSD, {})):
            for layers in (None, "greedy"):
                _refused(code, -2, "nbl_create_tems_wide", "(method 4)", method=method, max_iter=5, layers=layers, tems_wide=True, **extra)
        for flags in (2, 3, 0x80000000):
            rc, msg = _create_wide(code, None, flags)
            assert rc == -1 and "unknown flag bit" in msg and "NBL_TEMS_WIDE_LAYERED" in msg, (flags, rc, msg)
        rc, msg = _create_wide(code, nb.layer_greedy(code), 0)
        assert rc == -1 and "nbl_create_tems_wide" in msg and "layer_of = NULL" in msg, (rc, msg)
        # an invalid assignment keeps nbl_create_layered_ex's status and text
        bad, texts = np.zeros(code.M, dtype=np.int32), []
        for kw in (dict(damped=True), dict(tems_wide=True)):
            if "tems_wide" in kw or code.chk_deg.max() <= 8:              # (nbl_create_layered_ex itself refuses the degree-32 graph first)
                with pytest.raises(nb.NblError) as e:
                    nb.Decoder(code, layers=bad, **TEMS, **kw)
                assert e.value.status == -1 and "layered schedule: checks" in str(e.value) and "share variable" in str(e.value), str(e.value)
                texts.append(str(e.value))
        assert len(set(texts)) == 1, texts
    # everything else nbl_create refuses, with its text
    _refused(dc32, -1, "tems_nr < 1 or tems_nc < 0", method=nb.METHOD_TEMS, max_iter=5, tems_nr=0, tems_nc=2, tems_wide=True)
    _refused(dc32, -1, "tems_nr < 1 or tems_nc < 0", method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=-1, tems_wide=True)
    # nc above NBL_TEMS_WIDE_MAX_NC: refused where the wide programme must run (the text names both numbers), accepted where it need not
    for code in (dc32, profile_code("dc78", 64)[0]):
        for layers in (None, "greedy"):
            _refused(code, -2, "nbl_create_tems_wide", "tems_nc = 5", "above 4", method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=5, layers=layers, tems_wide=True)
            assert _past_every_check(*_create_wide(code, None, int(layers is not None), tems_nc=MAX_NC))
    assert _past_every_check(*_create_wide(nb.Code(GF16), None, 0, tems_nc=5))
    # the Python class refuses the options the entry point has no argument for; wide=True keeps meaning nbl_create_ems_wide
    for kw in (dict(osd_order=0), dict(bs_nm=4), dict(layers="greedy", damped=True), dict(layers="greedy", bp=True), dict(fht=True), dict(wide=True)):
        with pytest.raises(ValueError):
            nb.Decoder(dc32, tems_wide=True, **TEMS, **kw)
    _refused(dc32, -2, "nbl_create_ems_wide", "(method 2)", wide=True, **TEMS)


def test_lds_size_function_and_its_refusal():
    """[maxdc][q] dU and [q] Lc doubles, the DP states [2][nc + 1][q] of 16 bytes, min(nr, maxdc) (q - 1) list entries of 16 bytes, [q]
    ord01 and 3 maxdc + 4 words: the library's figure is that formula; a shape it puts above 160 KB is NBL_ERR_UNSUPPORTED with the byte
    count in the text, the one just below is accepted."""
    def formula(q, maxdc, nr, nc):
        return (maxdc * q + q) * 8 + 2 * (nc + 1) * q * 16 + min(nr, maxdc) * (q - 1) * 16 + q * 4 + (3 * maxdc + 4) * 4
    for shape in ((256, 32, 2, 3), (256, 32, 2, 4), (256, 32, 32, 2), (64, 32, 2, 3), (16, 10, 3, 4), (4, 2, 1, 0), (128, 17, 40, 2), (64, 8, 2, 3)):
        assert lds_bytes(*shape) == formula(*shape), shape
    assert lds_bytes(256, 32, 2, 3) == 109936                            # the issue's shape: one workgroup of four waves per CU
    assert lds_bytes(256, 16, 2, 3) == 76976 > 64 * 1024 >= lds_bytes(256, 9, 2, 2)      # the launchers opt in above 64 KB: both sides have GPU cases
    assert lds_bytes(256, 32, 15, 3) <= MAX_LDS < lds_bytes(256, 32, 16, 3)
    code = _ring_code(256, 20, 32)
    assert code.chk_deg.max() == 32
    for flags in (0, 1):
        assert _past_every_check(*_create_wide(code, None, flags, tems_nr=15, tems_nc=3)), flags
        for nr in (16, 32, 1000):
            rc, msg = _create_wide(code, None, flags, tems_nr=nr, tems_nc=3)
            assert rc == -2 and "nbl_create_tems_wide" in msg and str(lds_bytes(256, 32, nr, 3)) in msg and "LDS" in msg, (rc, msg)


def test_plan_names_the_wide_kernels():
    """A code with a check above degree 8 or with log2(q) maxdc > 32 -> tems_wide / tems_wide_layered under every debug switch; any other
    code gets the plan of nbl_create / nbl_create_layered_ex, fused kernels included, unless force_generic is 3 -- which leaves the plan
    alone where tems_nc > 4."""
    kw = dict(tems_nr=2, tems_nc=2)
    codes = [tc.wide_case(name)[0] for name in tc.NAMES] + [_ring_code(16, 20, 32), _graphs()[2]] + [profile_code(prof, q)[0] for prof, q in TEMS_REFUSED]
    for code in codes:
        assert code.chk_deg.max() > 8 or (code.q.bit_length() - 1) * int(code.chk_deg.max()) > 32
        for fg, rs in ((0, False), (1, False), (2, False), (3, False), (0, True), (3, True)):
            for nc in (2, MAX_NC):
                assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, force_generic=fg, record_state=rs, tems_nr=2, tems_nc=nc) == ("tems_wide", False, False, True)
                assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, layers="greedy", force_generic=fg, record_state=rs, tems_nr=2,
                                  tems_nc=nc) == ("tems_wide_layered", False, False, True)
    small = [profile_code("all", q)[0] for q in (4, 8, 16)] + [nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4), _ring_code(16, 12, 8),
                                                              _ring_code(128, 8, 4), profile_code("dv48", 256, "tems")[0]]
    names = set()
    for code in small:
        assert code.chk_deg.max() <= 8 and (code.q.bit_length() - 1) * int(code.chk_deg.max()) <= 32
        for nr_nc in (kw, dict(tems_nr=2, tems_nc=3), dict(tems_nr=3, tems_nc=5)):
            for fg, rs in ((0, False), (1, False), (2, False), (0, True), (2, True)):
                plain = debug_plan(code, nb.METHOD_TEMS, force_generic=fg, record_state=rs, **nr_nc)
                assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, force_generic=fg, record_state=rs, **nr_nc) == plain
                names.add(plain[0])
                plain = debug_plan(code, nb.METHOD_TEMS, layers="greedy", damped=True, force_generic=fg, record_state=rs, **nr_nc)
                assert plain == ("tems_layered", False, False, True)
                assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, layers="greedy", force_generic=fg, record_state=rs, **nr_nc) == plain
            for rs in (False, True):
                fusable = debug_plan(code, nb.METHOD_TEMS, **nr_nc)[1]
                if nr_nc["tems_nc"] <= MAX_NC:
                    assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, force_generic=3, record_state=rs, **nr_nc) == ("tems_wide", fusable, False, True)
                    assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, layers="greedy", force_generic=3, record_state=rs, **nr_nc) == ("tems_wide_layered", False, False, True)
                else:
                    assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, force_generic=3, record_state=rs, **nr_nc) == debug_plan(
                        code, nb.METHOD_TEMS, force_generic=3, record_state=rs, **nr_nc)
                    assert debug_plan(code, nb.METHOD_TEMS, tems_wide=True, layers="greedy", force_generic=3, record_state=rs, **nr_nc)[0] == "tems_layered"
            # the switch means nothing to a decoder of nbl_create
            assert debug_plan(code, nb.METHOD_TEMS, force_generic=3, **nr_nc)[0] in ("tems64", "tems256", "tems_small", "tems")
    assert {"tems64", "tems256", "tems"} <= names, names


@pytest.mark.parametrize("name", WIDE_SETS)
def test_wide_fixtures_literal_bit_exact(oracle, name):
    """The literal oracle equals the compiled reference bit for bit on T-EMS paths of 40 .. 192 bits: out, ret and syn_ok of every frame
    at every recorded iteration count, post / v2c / c2v of the recorded frame."""
    g, meta = load_golden(name)
    p = meta["spec"]["q"].bit_length() - 1
    assert meta["profile"]["method"] == 4 and p * max(meta["chk_degs"]) > 32
    assert meta["chk_degs"] == ([5, 8, 9, 16] if name == "deg_wide_gf256_tems" else [9, 12, 16, 17, 24, 32])
    assert list(g["iters"]) == [1, 2, 5, 12] and list(g["state_iters"]) == ([1] if name == "deg_wide_gf256_tems" else [1, 2])
    flags = g["syn_ok"][-1].tolist()
    assert 0 in flags and 1 in flags and g["syn_ok"][0].any() and not g["syn_ok"][0].all()      # at once, later and never
    tog._check_fixture(oracle, g, meta, name, oracle.LITERAL, True)


@pytest.mark.parametrize("name", WIDE_SETS)
def test_wide_fixtures_canonical_matches_reference_decisions(oracle, name):
    """The canonical oracle gives the compiled reference's decisions, flags and iteration counts on every frame; its state differs by the
    reference's add-then-subtract residue only, held to the 1e-9 relative tolerance tests/test_oracle_golden.py applies (measured, largest
    absolute difference over the recorded state: 8.8e-13 at GF(64), 1.1e-13 at GF(16) shaped, 8.4e-12 at GF(256))."""
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
    wide = [9, 12, 16, 17, 24, 32]
    want = {"gf64-nc2": wide, "gf64-nc3": wide, "gf16-shaped": wide, "gf4-nr1": wide, "gf64-dc6-8": [6, 7, 8], "gf256-dc5-9": [5, 6, 8, 9],
            "gf256-dc17": [9, 12, 16, 17], "gf256-dc32": [9, 16, 32], "gf128-mix": [2, 3, 4, 8, 9, 10, 31, 32], "gf16-nc4": [9, 10]}
    assert set(want) == set(tc.NAMES)
    for name in tc.NAMES:
        code, kw, L = tc.wide_case(name)
        assert sorted(set(code.chk_deg.tolist())) == want[name] and code.N <= 88 and L.shape[0] <= tc.B_BATCH, name
        assert sorted(set(code.var_deg.tolist())) == ([1, 2, 3, 8] if name == "gf128-mix" else [2, 3]), name
        assert kw["tems_nc"] <= MAX_NC and lds_bytes(code.q, int(code.chk_deg.max()), kw["tems_nr"], kw["tems_nc"]) <= MAX_LDS
        assert code.chk_deg.max() > 8 or (code.q.bit_length() - 1) * int(code.chk_deg.max()) > 32
    assert tc.wide_case("gf4-nr1")[1] == dict(tems_nr=1, tems_nc=4) and tc.wide_case("gf16-nc4")[1]["tems_nc"] == MAX_NC
    assert tc.wide_case("gf64-dc6-8")[0].chk_deg.max() == 8               # inside the degree limit of nbl_create, outside its path code


@pytest.mark.parametrize("fixed", [0, 1])
@pytest.mark.parametrize("which", tc.SCHEDULES)
@pytest.mark.parametrize("name", tc.NAMES)
def test_conditions_on_every_gpu_case(oracle, name, which, fixed):
    """Under the canonical oracle at least one frame of the case converges at iteration 1, at least one later and at least one never
    within MAX_ITER; no decision is a tie; some check node ran.  Fixed iterations freeze the same outputs at the same counts."""
    ref = tc.wide_reference(name, which, fixed)
    flags = [(r[1], r[2]) for r in ref]
    print(name, which, fixed, flags, "smallest margin", min(tc.margin(r[3]) for r in ref))
    assert (1, 1) in flags and any(c and 1 < i <= tc.MAX_ITER for c, i in flags) and (0, tc.MAX_ITER) in flags, flags
    for b, r in enumerate(ref):
        assert tc.margin(r[3]) > 0.0, (name, which, b)
        assert np.all(np.isfinite(r[3])) and np.all(np.isfinite(r[4])) and np.all(np.isfinite(r[5])), b
        assert r[4].any() or (r[2] == 1 and not fixed), b
    if fixed:
        early = tc.wide_reference(name, which, 0)
        assert [(r[1], r[2]) for r in early] == flags and all(np.array_equal(a[0], b[0]) for a, b in zip(ref, early))


def test_the_ties_frames_discriminate_the_rule_for_equal_costs(oracle):
    """On the integer-valued frames of the GPU ties test the restated DP (tests/tems_wide_ref.py) with "the first path in enumeration
    order wins among equal costs" reproduces the oracle's check node bit for bit on every check, and with "the last" it does not on most:
    the frames see the path comparison."""
    code, kw, _ = tc.wide_case(tc.TIES_CASE)
    od, gf = tc.oracle_decoder(tc.TIES_CASE, 1, 1, tuple(sorted(kw.items())))
    L = tc.ties_frames()
    assert np.array_equal(L, np.round(L)) and L.min() >= -3 and L.max() <= 1
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    first = last = 0
    for m in range(code.M):
        vin, h = L[0][code.chk_var[off[m]:off[m + 1]]], code.chk_h[off[m]:off[m + 1]]
        ref = od.check(m, vin)
        first += np.array_equal(tems_wide_ref.check_node(vin, h, gf.mul, kw["tems_nr"], kw["tems_nc"], tie="first"), ref)
        last += np.array_equal(tems_wide_ref.check_node(vin, h, gf.mul, kw["tems_nr"], kw["tems_nc"], tie="last"), ref)
    print("checks equal to the oracle: first", first, "last", last, "of", code.M)
    assert first == code.M and last < code.M // 2
