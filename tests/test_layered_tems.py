"""The damped layered (check-serial) T-EMS schedule without a GPU: the refusals and acceptances of nbl_create_layered_ex, and the
numpy restatement (tests/layered_tems_ref.py) on the very cases the GPU tests compare with (tests/test_gpu_layered_tems.py imports
case() and reference() from here, so each reference is computed once per process)."""
import concurrent.futures
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import layered_ref as lr
import layered_tems_ref as ltr
import pyoracle
from degree_util import profile_code
from test_abi import _no_device, _ring_code
from test_gpu_layered import assignments
from test_gpu_parity import _bpsk_llr_zero
from test_layered import EMS, GF16, _refused, oracle_edges

TEMS = dict(method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=3)


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, kw, L, max_iter) of a named case; built once"""
    if name == "gf16":
        # all-zero codeword over BPSK at 1.5 dB, chosen on the CPU with the restatement alone: frames 4, 6 and 7 converge at iterations
        # 6, 3 and 4 and the other five do not (asserted in test_gpu_layered_tems.py)
        code = nb.Code(GF16)
        return code, dict(tems_nr=2, tems_nc=3), _bpsk_llr_zero(np.random.default_rng(77), code, 8, 1.5), 6
    if name in ("ring256", "ring64"):
        q = int(name[4:])
        code = _ring_code(q, 8, 4)
        L = np.random.default_rng(q).normal(-1.5, 3.0, (4, code.N, q - 1))
        L[1, ::3] = 0.0                                 # every third symbol erased
        return code, dict(tems_nr=2, tems_nc=3, tems_factor=1.15, tems_offset=0.2), L, 4
    prof, q, nr, nc = name.split("-")                   # <profile>-<q>-<nr>-<nc>
    q, nr, nc = int(q), int(nr), int(nc)
    code = profile_code(prof, q, method="tems")[0]
    frames = 1 if prof == "all" or q == 256 else 2
    L = np.random.default_rng(100 * q + 10 * nr + nc).normal(-1.5, 3.0, (frames, code.N, q - 1))
    if prof == "all":
        L = np.round(L)                                 # an integer grid: exact ties (factor 1, offset 0: every sum is exact)
    return code, dict(tems_nr=nr, tems_nc=nc), L, 4


CASES = (("gf16", ("greedy",)), ("ring256", ("greedy", "serial", "other")), ("ring64", ("greedy", "serial", "other")),
         ("all-4-2-4", ("greedy",)), ("all-8-2-4", ("greedy",)), ("all-16-2-4", ("greedy",)),
         ("all-4-1-3", ("greedy",)), ("all-8-1-3", ("greedy",)), ("all-16-1-3", ("greedy",)),
         ("dv48-32-2-3", ("greedy",)), ("dv48-256-2-3", ("greedy",)))


@functools.lru_cache(maxsize=None)
def reference(name, which, fixed=0, damp=True, frames=None):
    """[(out, converged, iters, post, c2v, v2c, visits, blends)] per frame (`frames`: of the first so many) of a case under assignment
    `which`; computed once and shared.  The time goes into the oracle's check-node update at GF(256), which leaves the interpreter lock
    alone: one oracle decoder and one thread per frame."""
    code, kw, L, iters = case(name)
    ocode = pyoracle.Code(edges=oracle_edges(code))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    gf = pyoracle.GF(code.q)
    layer_of = assignments(code)[which]

    def one(b):
        od = pyoracle.Decoder(ocode, gf, pyoracle.TEMS, iters, pyoracle.CANONICAL, fixed_iters=fixed, **kw)
        return ltr.decode(od, gf.mul, L[b], layer_of, iters, fixed_iters=fixed, damp=damp)

    B = L.shape[0] if frames is None else frames
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(B, 8)) as pool:
        return list(pool.map(one, range(B)))


def test_create_layered_ex_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    # ---- flags = 0 IS nbl_create_layered: every refusal tests/test_layered.py pins, the same status and text ----
    bad = greedy.copy()
    bad[3] = -1
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad, damped=False, **EMS)
    bad = greedy.copy()
    bad[bad == bad.max()] += 1
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad, damped=False, **EMS)
    bad = greedy.copy()
    bad[5] = 1 << 30
    _refused(code, -1, "empty layer", layers=bad, damped=False, **EMS)
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    v = int(code.chk_var[0])
    other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
    shared = greedy.copy()
    shared[other] = shared[0]
    _refused(code, -1, "checks ", " share variable ", layers=shared, damped=False, **EMS)
    for method in (nb.METHOD_BP, nb.METHOD_TEMS, nb.METHOD_BS_TEMS, nb.METHOD_OSD, 3, 0):
        _refused(code, -2, "layered schedule is defined for EMS", layers="greedy", damped=False, method=method, max_iter=5)
        _refused(code, -2, "layered schedule is defined for EMS", layers=greedy, damped=False, method=method, max_iter=5)
    _refused(code, -1, "EMS_Nm is too large", layers="greedy", damped=False, method=nb.METHOD_EMS, max_iter=5, ems_nm=17)
    _refused(_ring_code(512, 8, 4), -2, "GF(256)", layers="greedy", damped=False, gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **EMS)
    broken = nb.Code(GF16)
    broken.var_h = broken.var_h.copy()
    broken.var_h[0] ^= 1
    _refused(broken, -1, "disagree", layers="greedy", damped=False, **EMS)
    # ---- an unknown flag bit ----
    for flags in (2, 3, 1 << 31):
        _refused(code, -1, "unknown flag bit", layers="greedy", damped=flags, **TEMS)
        _refused(code, -1, "unknown flag bit", layers="greedy", damped=flags, **EMS)
    # ---- NBL_LAYERED_DAMPED: the methods that stay out; the message names what is served ----
    for method in (nb.METHOD_BP, nb.METHOD_BS_TEMS, nb.METHOD_OSD, 3, 0):
        _refused(code, -2, "NBL_LAYERED_DAMPED", "T-EMS (method 4)", "EMS (method 2)", layers="greedy", damped=True, method=method, max_iter=5)
        _refused(code, -2, "T-EMS (method 4)", layers=greedy, damped=True, method=method, max_iter=5)
    # ---- everything nbl_create refuses is refused the same way: the 32-bit path code, the parameters, the graph ----
    wide = profile_code("all", 32)[0]
    assert 5 * wide.chk_deg.max() > 32
    _refused(wide, -2, "must not exceed 32", layers="greedy", damped=True, **TEMS)
    _refused(code, -1, "tems_nr < 1", layers="greedy", damped=True, method=nb.METHOD_TEMS, max_iter=5, tems_nr=0)
    _refused(broken, -1, "disagree", layers="greedy", damped=True, **TEMS)
    _refused(code, -1, "EMS_Nm is too large", layers="greedy", damped=True, method=nb.METHOD_EMS, max_iter=5, ems_nm=17)
    # ---- a bad assignment, with the flag, on both methods it serves ----
    for prm in (TEMS, EMS):
        _refused(code, -1, "checks ", " share variable ", layers=shared, damped=True, **prm)
        bad = greedy.copy()
        bad[3] = -1
        _refused(code, -1, "layer_of[3]", "below 0", layers=bad, damped=True, **prm)
    # ---- more than 160 KB of LDS per check: at creation, not at the first decode (GF(256), degree 4, nc = 40: 41 cost rows) ----
    _refused(_ring_code(256, 8, 4), -2, "T-EMS", "160 KB", layers="greedy", damped=True, method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=40)
    # ---- the Python layer: damped belongs to layers ----
    with pytest.raises(ValueError):
        nb.Decoder(code, damped=True, **TEMS)


def test_create_layered_ex_accepts_valid_requests():
    """The checks of nbl_create_layered_ex precede the device: an accepted request fails with NBL_ERR_NO_DEVICE on a box without a GPU
    and makes a decoder on one."""
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    big = _ring_code(256, 8, 4)
    for c, kw in ((code, dict(layers="greedy", damped=True, **TEMS)), (code, dict(layers=greedy, damped=True, **TEMS)),
                  (code, dict(layers=np.arange(code.M), damped=True, **TEMS)), (code, dict(layers="greedy", damped=True, **EMS)),
                  (code, dict(layers="greedy", damped=False, **EMS)), (big, dict(layers="greedy", damped=True, **{**TEMS, "tems_nc": 9})),
                  (profile_code("all", 16)[0], dict(layers="greedy", damped=True, **{**TEMS, "tems_nc": 4}))):
        if _no_device():
            _refused(c, -3, "no CPU decode path", **kw)
        else:
            dec = nb.Decoder(c, **kw)
            want = nb.layer_greedy(c) if isinstance(kw["layers"], str) else np.asarray(kw["layers"])
            assert np.array_equal(dec.layers, want)
            dec.close()


@pytest.mark.parametrize("name,whiches", CASES, ids=[c[0] for c in CASES])
def test_every_case_takes_the_blend_sometimes(oracle, name, whiches):
    """What keeps the GPU tests from hiding a missing damping: in every case, under every assignment used, every frame takes the blend
    at least once and not on every edge visit, and the result differs from the undamped one.  On the ring codes the three assignments
    give three different results."""
    refs = {w: reference(name, w) for w in whiches}
    for w, ref in refs.items():
        for b, r in enumerate(ref):
            visits, blends = r[6], r[7]
            print(name, w, b, "blends", blends, "of", visits, "converged", r[1], "iters", r[2])
            assert 0 < blends < visits, (name, w, b, blends, visits)
            assert np.all(np.isfinite(r[4])) and np.all(np.isfinite(r[5]))
    # the undamped run: under the greedy assignment only, and at GF(256) on frame 0 only (seconds of oracle time per frame there).
    # A frame whose few blends all come early can end in the same state (the erased frame of the ring codes does: 6 blends of 128
    # visits); every other frame must not.
    code = case(name)[0]
    plain = reference(name, "greedy", damp=False, frames=1 if code.q == 256 else None)
    differs = [not (np.array_equal(r[4], p[4]) and np.array_equal(r[5], p[5])) for r, p in zip(refs["greedy"], plain)]
    assert all(p[7] == 0 for p in plain)
    assert differs[0] and sum(differs) >= len(differs) - 1, (name, differs)
    if len(whiches) == 3:
        for a, b in (("greedy", "serial"), ("greedy", "other"), ("serial", "other")):
            assert any(not np.array_equal(x[4], y[4]) for x, y in zip(refs[a], refs[b])), (name, a, b)
            assert any(not np.array_equal(x[5], y[5]) for x, y in zip(refs[a], refs[b])), (name, a, b)


def test_one_iteration_equals_the_flooding_oracle(oracle):
    """Iteration 1 decides from L_ch alone, whatever the schedule; and before any check has run, v2c = L_ch of the edge's variable."""
    code, kw, L, _ = case("gf16")
    ocode = oracle.Code(edges=oracle_edges(code))
    gf = oracle.GF(code.q)
    od = oracle.Decoder(ocode, gf, oracle.TEMS, 1, oracle.CANONICAL, **kw)
    edge_var = np.repeat(np.arange(code.N), code.var_deg)
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        out, conv, iters, post, c2v, v2c, _, _ = ltr.decode(od, gf.mul, L[b], lr.greedy_layers(code.chk_deg, code.chk_var), 1)
        assert (conv, iters) == (r, it) and np.array_equal(out, o), b
        assert np.array_equal(post, od.state()[0]), b
        if conv:                                        # the frame ended before its first layer: the state of "iteration 0"
            assert not c2v.any() and np.array_equal(v2c, L[b][edge_var]), b
