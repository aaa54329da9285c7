"""The damped layered (check-serial) log-QSPA schedule without a GPU: the refusals and acceptances of nbl_create_layered_bp, the plan,
and the numpy restatement (tests/layered_bp_ref.py) on the very cases the GPU tests compare with (tests/test_gpu_layered_bp.py imports
case() and reference() from here, so each reference is computed once per process)."""
import concurrent.futures
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import layered_ref as lr
import layered_bp_ref as lbr
import pyoracle
from degree_util import profile_code
from nbldpc_amd.binding import debug_plan
from test_abi import _no_device, _ring_code
from test_gpu_layered import assignments
from test_gpu_parity import _bpsk_llr_zero, _random_code
from test_layered import GF16, _refused, oracle_edges

BP = dict(method=nb.METHOD_BP, max_iter=5)
GAP_MIN = 1e-6      # smallest decide gap a case may have (layered_bp_ref.py): three orders above the 1e-9 the LLRs agree to

# seeds of the synthetic inputs, chosen on the CPU with the restatement alone until every case's smallest decide gap is above GAP_MIN
# (test_every_gpu_case_decides_with_a_margin); a condition on the inputs, not on any kernel
SEEDS = {"ring256": 256, "ring64": 64, "all-4": 4, "all-8": 8, "all-16": 16, "dv48-32": 32, "rand128": 128}


def _frames(rng, N, q, kinds):
    """one frame per kind: n = normal(-2, 4); w = normal(-900, 700), the mantissa / exponent path of the convolutions; m = narrow and
    wide vectors mixed in one check (frame 5 of tests/test_gpu_parity.py::test_small_field_bp_vs_oracle).  No all-zero and no partly
    erased frame: see that test's docstring."""
    L = np.empty((len(kinds), N, q - 1))
    for b, kind in enumerate(kinds):
        if kind == "n":
            L[b] = rng.normal(-2, 4, (N, q - 1))
        elif kind == "w":
            L[b] = rng.normal(-900, 700, (N, q - 1))
        else:
            L[b] = rng.normal(-2, 3, (N, q - 1)) * np.where(rng.random((N, 1)) < 0.5, 1.0, 2000.0)
    return L


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, L, max_iter) of a named case; built once"""
    if name in ("gf16", "gf16-2db"):
        # all-zero codeword over BPSK at 1.5 dB (2.0 dB), chosen on the CPU with the restatement alone: at 1.5 dB frames 3, 4, 6 and 7
        # converge at iterations 7, 4, 2 and 4 and the other four do not within 8 (asserted below)
        code = nb.Code(GF16)
        return (code, _bpsk_llr_zero(np.random.default_rng(77), code, 8, 1.5), 8) if name == "gf16" else \
               (code, _bpsk_llr_zero(np.random.default_rng(77), code, 8, 2.0), 30)
    rng = np.random.default_rng(SEEDS[name])
    if name in ("ring256", "ring64"):
        q = int(name[4:])
        code = _ring_code(q, 8, 4)
        return code, _frames(rng, code.N, q, "nwm"), 3
    if name == "rand128":
        code = _random_code(128, 1128)[0]
        return code, _frames(rng, code.N, 128, "n"), 3
    prof, q = name.split("-")                           # <profile>-<q>
    code = profile_code(prof, int(q))[0]
    return code, _frames(rng, code.N, int(q), "n"), 3


CASES = (("gf16", ("greedy",)), ("ring256", ("greedy", "serial", "other")), ("ring64", ("greedy", "serial", "other")),
         ("all-4", ("greedy",)), ("all-8", ("greedy",)), ("all-16", ("greedy",)), ("dv48-32", ("greedy",)), ("rand128", ("greedy",)))


@functools.lru_cache(maxsize=None)
def reference(name, which, fixed=0, damp=True):
    """[(out, converged, iters, post, c2v, v2c, visits, blends, gap)] per frame of a case under assignment `which`; computed once and
    shared.  The time goes into the oracle's check-node update, which leaves the interpreter lock alone: one oracle decoder and one
    thread per frame."""
    code, L, iters = case(name)
    ocode = pyoracle.Code(edges=oracle_edges(code))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    gf = pyoracle.GF(code.q)
    layer_of = assignments(code)[which]

    def one(b):
        od = pyoracle.Decoder(ocode, gf, pyoracle.BP, iters, pyoracle.CANONICAL, fixed_iters=fixed)
        return lbr.decode(od, gf.mul, L[b], layer_of, iters, fixed_iters=fixed, damp=damp)

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(L.shape[0], 8)) as pool:
        return list(pool.map(one, range(L.shape[0])))


@functools.lru_cache(maxsize=None)
def flooding(name):
    """[(converged, iters, c2v)] per frame of a case under the oracle's flooding log-QSPA (nblo_decode, CANONICAL)"""
    code, L, iters = case(name)
    od = pyoracle.Decoder(pyoracle.Code(edges=oracle_edges(code)), pyoracle.GF(code.q), pyoracle.BP, iters, pyoracle.CANONICAL)
    ref = []
    for b in range(L.shape[0]):
        r, _, it = od.decode(L[b])
        ref.append((r, it, od.state()[2].copy()))
    return ref


def test_create_layered_bp_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    # ---- every assignment error of nbl_create_layered, with its status and text ----
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    v = int(code.chk_var[0])
    other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
    shared = greedy.copy()
    shared[other] = shared[0]
    first = next((m, int(x)) for m in range(code.M) for x in code.chk_var[off[m]:off[m + 1]]
                 if any(shared[k] == shared[m] and int(x) in code.chk_var[off[k]:off[k + 1]].tolist() for k in range(m)))
    partner = next(k for k in range(first[0]) if shared[k] == shared[first[0]] and first[1] in code.chk_var[off[k]:off[k + 1]].tolist())
    _refused(code, -1, f"checks {partner} and {first[0]} ", f"share variable {first[1]}", layers=shared, bp=True, **BP)
    bad = greedy.copy()
    bad[3] = -1
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad, bp=True, **BP)
    bad = greedy.copy()
    bad[bad == bad.max()] += 1
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad, bp=True, **BP)
    bad = greedy.copy()
    bad[5] = 1 << 30
    _refused(code, -1, "empty layer", layers=bad, bp=True, **BP)
    # ---- any method but 1: the message names method 1 and points to the other two entry points ----
    for method in (nb.METHOD_EMS, nb.METHOD_TEMS, nb.METHOD_OSD, nb.METHOD_BS_TEMS, 3, 0):
        for layers in ("greedy", greedy):
            _refused(code, -2, "log-QSPA (method 1)", "nbl_create_layered", "nbl_create_layered_ex", layers=layers, bp=True, method=method, max_iter=5)
    # ---- everything nbl_create refuses, the same way ----
    _refused(code, -1, "max_iter < 0", layers="greedy", bp=True, method=nb.METHOD_BP, max_iter=-1)
    _refused(_ring_code(512, 8, 4), -2, "GF(256)", layers="greedy", bp=True, gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **BP)
    broken = nb.Code(GF16)
    broken.var_h = broken.var_h.copy()
    broken.var_h[0] ^= 1
    _refused(broken, -1, "disagree", layers="greedy", bp=True, **BP)
    broken = nb.Code(GF16)
    broken.chk_h = broken.chk_h.copy()
    broken.chk_h[2] = 0
    _refused(broken, -1, "zero coefficient", layers="greedy", bp=True, **BP)
    mul, inv = (np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(16))
    bad_mul = mul.copy()
    bad_mul[3, 5] ^= 1
    with pytest.raises(nb.NblError) as e:
        nb.Decoder(code, layers="greedy", bp=True, gf=(bad_mul, inv), **BP)
    assert e.value.status == -1
    with pytest.raises(nb.NblError) as f:
        nb.Decoder(code, gf=(bad_mul, inv), **BP)
    assert (f.value.status, str(f.value)) == (e.value.status, str(e.value))
    # ---- the flag route stays closed (tests/test_layered_tems.py pins the same) ----
    _refused(code, -1, "unknown flag bit", layers="greedy", damped=2, **BP)
    _refused(code, -2, "NBL_LAYERED_DAMPED", layers="greedy", damped=True, **BP)
    _refused(code, -2, "layered schedule is defined for EMS", layers="greedy", **BP)
    # ---- the Python layer: bp belongs to layers, and takes no flags ----
    with pytest.raises(ValueError):
        nb.Decoder(code, bp=True, **BP)
    with pytest.raises(ValueError):
        nb.Decoder(code, layers="greedy", damped=True, bp=True, **BP)
    with pytest.raises(ValueError):
        nb.Decoder(code, layers="greedy", damped=False, bp=True, **BP)


def test_create_layered_bp_accepts_valid_requests():
    """The checks of nbl_create_layered_bp precede the device: an accepted request fails with NBL_ERR_NO_DEVICE on a box without a GPU
    and makes a decoder on one.  The largest shape of the envelope (GF(256), check degree 8: 59,392 B of LDS) is accepted."""
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    for c, layers in ((code, "greedy"), (code, greedy), (code, np.arange(code.M)), (code, greedy.max() - greedy),
                      (_ring_code(256, 12, 8), "greedy"), (profile_code("all", 256)[0], "greedy")):
        kw = dict(layers=layers, bp=True, **BP)
        if _no_device():
            _refused(c, -3, "no CPU decode path", **kw)
        else:
            dec = nb.Decoder(c, **kw)
            assert np.array_equal(dec.layers, nb.layer_greedy(c) if isinstance(layers, str) else np.asarray(layers))
            dec.close()


def test_gf16_iterations_blends_and_what_the_state_depends_on(oracle):
    """The `gf16` case (8 frames at 1.5 dB, 8 iterations, greedy): where each frame converges; the blend is taken sometimes and not
    always; without the damping the state differs; and it differs from flooding's."""
    ref = reference("gf16", "greedy")
    assert [(r[1], r[2]) for r in ref] == [(0, 8), (0, 8), (0, 8), (1, 7), (1, 4), (0, 8), (1, 2), (1, 4)]
    plain, flood = reference("gf16", "greedy", damp=False), flooding("gf16")
    for b, (r, p, f) in enumerate(zip(ref, plain, flood)):
        print("gf16", b, "blends", r[7], "of", r[6], "gap", r[8], "flooding", f[:2])
        assert 0 < r[7] < r[6], b
        assert p[7] == 0 and np.all(np.isfinite(r[4])) and np.all(np.isfinite(r[5]))
        assert not np.array_equal(r[4], f[2]), b
    assert all(not np.array_equal(r[4], p[4]) or not np.array_equal(r[5], p[5]) for r, p in zip(ref, plain) if r[2] > 2)
    assert [(f[0], f[1]) for f in flood] != [(r[1], r[2]) for r in ref]


def test_gf16_at_2db_needs_fewer_iterations_than_flooding(oracle):
    """2.0 dB, up to 30 iterations: every frame converges under both schedules, the layered one sooner on every frame."""
    ref, flood = reference("gf16-2db", "greedy"), flooding("gf16-2db")
    assert [f[:2] for f in flood] == [(1, i) for i in (5, 8, 13, 5, 5, 11, 3, 5)]
    assert [(r[1], r[2]) for r in ref] == [(1, i) for i in (4, 5, 5, 4, 3, 8, 2, 3)]
    assert min(r[8] for r in ref) > GAP_MIN


@pytest.mark.parametrize("name,whiches", CASES, ids=[c[0] for c in CASES])
def test_every_gpu_case_decides_with_a_margin(oracle, name, whiches):
    """A condition on the inputs alone: in every case the GPU tests use, under every assignment and in fixed-iteration mode where they
    use it, no DecideLLRVector call of the restatement has its two best candidates closer than 1e-6 -- so decisions, flags and
    iteration counts cannot hang on the 1e-9 the LLRs agree to (tests/test_gpu_parity.py::test_small_field_bp_vs_oracle says why no
    all-zero or partly erased frame is among them).  Every frame runs its checks at least once, with finite results; the three
    assignments of the ring codes give three different states."""
    refs = {w: reference(name, w) for w in whiches}
    if name == "gf16":
        refs["fixed"] = reference(name, "greedy", 1)
    for w, ref in refs.items():
        for b, r in enumerate(ref):
            print(name, w, b, "gap", r[8], "blends", r[7], "of", r[6], "converged", r[1], "iters", r[2])
            assert r[8] > GAP_MIN, (name, w, b, r[8])
            assert r[6] > 0 and np.all(np.isfinite(r[4])) and np.all(np.isfinite(r[5])) and np.any(r[4] != 0.0), (name, w, b)
    if len(whiches) == 3:
        for a, b in (("greedy", "serial"), ("greedy", "other"), ("serial", "other")):
            assert any(not np.array_equal(x[4], y[4]) for x, y in zip(refs[a], refs[b])), (name, a, b)


def test_one_iteration_equals_the_flooding_oracle(oracle):
    """Iteration 1 decides from L_ch alone, whatever the schedule; and before any check has run, v2c = L_ch of the edge's variable."""
    code, L, _ = case("gf16")
    ocode = oracle.Code(edges=oracle_edges(code))
    gf = oracle.GF(code.q)
    od = oracle.Decoder(ocode, gf, oracle.BP, 1, oracle.CANONICAL)
    edge_var = np.repeat(np.arange(code.N), code.var_deg)
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        out, conv, iters, post, c2v, v2c = lbr.decode(od, gf.mul, L[b], lr.greedy_layers(code.chk_deg, code.chk_var), 1)[:6]
        assert (conv, iters) == (r, it) and np.array_equal(out, o), b
        assert np.array_equal(post, od.state()[0]), b
        if conv:
            assert not c2v.any() and np.array_equal(v2c, L[b][edge_var]), b


def test_plan_names_the_layered_bp_kernel():
    """(method 1, layered) -> bp_layered, never fused, v2c kept, in every variant; the layered kinds of the other methods and flooding
    log-QSPA stay what tests/test_plan.py pins."""
    for code in (nb.Code(GF16), _ring_code(256, 8, 4), _ring_code(64, 8, 4), profile_code("all", 8)[0]):
        for fg, rs in ((0, False), (1, False), (2, False), (0, True)):
            assert debug_plan(code, nb.METHOD_BP, layers="greedy", force_generic=fg, record_state=rs) == ("bp_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_EMS, ems_nm=4, layers="greedy") == ("ems_layered", False, False, False)
        assert debug_plan(code, nb.METHOD_TEMS, layers="greedy", damped=True) == ("tems_layered", False, False, True)
        assert debug_plan(code, nb.METHOD_BP)[0] in ("bp256", "bp64", "bp_small", "bp")
        assert debug_plan(code, nb.METHOD_BP, force_generic=1)[0] == "bp"
