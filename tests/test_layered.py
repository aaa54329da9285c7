"""The layered (check-serial) EMS schedule without a GPU: the default layer assignment, the refusals of nbl_create_layered, and the
numpy restatement (tests/layered_ref.py) that the GPU tests compare with."""
import numpy as np
import pytest

import nbldpc_amd as nb
import layered_ref as lr
from degree_util import profile_code
from test_abi import _no_device, _ring_code

GF16 = "divsalar.UNBLDPC.128.64.GF.16"
EMS = dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2)


def oracle_edges(code):
    """(N, M, q, edge_var, edge_chk, edge_h) in variable-major order, what pyoracle.Code takes"""
    return code.N, code.M, code.q, np.repeat(np.arange(code.N, dtype=np.int32), code.var_deg), code.var_chk, code.var_h


def graphs():
    for name in sorted(nb.datafiles.codes()):
        yield name, nb.Code(name)
    for q in (4, 16, 256):
        yield f"ring{q}", _ring_code(q, 8, 4)
        yield f"ring{q}-dc8", _ring_code(q, 12, 8)
        yield f"all{q}", profile_code("all", q)[0]


def test_greedy_layers_equal_the_python_colouring():
    """nbl_layer_greedy on the ten shipped codes, ring graphs and the `all` degree profile (checks 2-8, variables 1-8) for q = 4, 16,
    256: the same assignment as the pure-Python colouring, every layer non-empty, no two checks of a layer sharing a variable."""
    n = 0
    for tag, code in graphs():
        got = nb.layer_greedy(code)
        assert got.dtype == np.int32 and got.shape == (code.M,)
        assert np.array_equal(got, lr.greedy_layers(code.chk_deg, code.chk_var)), tag
        assert lr.layers_valid(code.chk_deg, code.chk_var, got), tag
        assert 1 < got.max() + 1 < code.M, tag          # (neither flooding nor one layer per check on any of these)
        n += 1
    assert n == 10 + 9
    # the validity check used above can fail: two neighbours in one layer, a gap
    code = _ring_code(16, 8, 4)
    bad = nb.layer_greedy(code).copy()
    bad[1] = bad[0]                                     # (variable 0 joins checks 0 and 1)
    assert not lr.layers_valid(code.chk_deg, code.chk_var, bad)
    assert not lr.layers_valid(code.chk_deg, code.chk_var, np.arange(code.M) * 2)


def _refused(code, status, *words, **kw):
    with pytest.raises(nb.NblError) as e:
        nb.Decoder(code, **kw)
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_create_layered_refusals_come_before_the_device():
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    # two checks of one layer sharing a variable: the message names both checks and the variable
    off = np.concatenate([[0], np.cumsum(code.chk_deg)])
    v = int(code.chk_var[0])
    other = next(m for m in range(1, code.M) if v in code.chk_var[off[m]:off[m + 1]].tolist())
    bad = greedy.copy()
    bad[other] = bad[0]
    first = next((m, int(x)) for m in range(code.M) for x in code.chk_var[off[m]:off[m + 1]]
                 if any(bad[k] == bad[m] and int(x) in code.chk_var[off[k]:off[k + 1]].tolist() for k in range(m)))
    partner = next(k for k in range(first[0]) if bad[k] == bad[first[0]] and first[1] in code.chk_var[off[k]:off[k + 1]].tolist())
    _refused(code, -1, f"checks {partner} and {first[0]} ", f"share variable {first[1]}", layers=bad, **EMS)
    # a negative layer
    bad = greedy.copy()
    bad[3] = -1
    _refused(code, -1, "layer_of[3]", "below 0", layers=bad, **EMS)
    # an empty layer below the largest index used
    bad = greedy.copy()
    bad[bad == bad.max()] += 1
    _refused(code, -1, f"layer {greedy.max()} is empty", layers=bad, **EMS)
    bad = greedy.copy()
    bad[5] = 1 << 30
    _refused(code, -1, "empty layer", layers=bad, **EMS)
    # methods 1, 4 and 7 (and the ones nothing decodes): defined for EMS only
    for method in (nb.METHOD_BP, nb.METHOD_TEMS, nb.METHOD_BS_TEMS, nb.METHOD_OSD, 3, 0):
        _refused(code, -2, "layered schedule is defined for EMS", layers="greedy", method=method, max_iter=5)
        _refused(code, -2, "layered schedule is defined for EMS", layers=greedy, method=method, max_iter=5)
    # everything nbl_create refuses is refused the same way
    _refused(code, -1, "EMS_Nm is too large", layers="greedy", method=nb.METHOD_EMS, max_iter=5, ems_nm=17)
    _refused(_ring_code(512, 8, 4), -2, "GF(256)", layers="greedy", gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)), **EMS)
    broken = nb.Code(GF16)
    broken.var_h = broken.var_h.copy()
    broken.var_h[0] ^= 1
    _refused(broken, -1, "disagree", layers="greedy", **EMS)
    # nbl_layer_greedy itself: an edge that points outside the graph
    broken = nb.Code(GF16)
    broken.chk_var = broken.chk_var.copy()
    broken.chk_var[7] = broken.N
    with pytest.raises(nb.NblError) as e:
        nb.layer_greedy(broken)
    assert e.value.status == -1 and "out of range" in str(e.value)


def test_create_layered_accepts_valid_requests():
    """The checks of nbl_create_layered precede the device (tests/test_abi.py::_accepted): an accepted request fails with
    NBL_ERR_NO_DEVICE on a box without a GPU and makes a decoder on one."""
    code = nb.Code(GF16)
    greedy = nb.layer_greedy(code)
    big = _ring_code(256, 12, 8)
    for c, kw in ((code, dict(layers="greedy")), (code, dict(layers=greedy)), (code, dict(layers=np.arange(code.M))),
                  (code, dict(layers=greedy.max() - greedy)), (big, dict(layers="greedy", ems_nm=256, ems_nc=6))):
        kw = {**EMS, **kw}
        if _no_device():
            _refused(c, -3, "no CPU decode path", **kw)
        else:
            dec = nb.Decoder(c, **kw)
            want = nb.layer_greedy(c) if isinstance(kw["layers"], str) else np.asarray(kw["layers"])
            assert np.array_equal(dec.layers, want)
            dec.close()


@pytest.fixture(scope="module")
def gf16(oracle):
    code = nb.Code(GF16)
    ocode = oracle.Code(edges=oracle_edges(code))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    rng = np.random.default_rng(2024)
    L = rng.normal(-1.0, 3.0, (4, code.N, code.q - 1))
    L[1] = -np.abs(L[1])                                # nothing positive: the all-zero word, zero syndrome at iteration 1
    return code, ocode, oracle.GF(code.q), L


def test_one_iteration_equals_the_flooding_oracle(oracle, gf16):
    """Iteration 1 decides from L_ch alone, whatever the schedule: with max_iter = 1 the restatement's out / converged / iters are the
    flooding oracle's, for every assignment."""
    code, ocode, gf, L = gf16
    od = oracle.Decoder(ocode, gf, oracle.EMS, 1, oracle.CANONICAL, ems_nm=8, ems_nc=3)
    flags = []
    for layer_of in (lr.greedy_layers(code.chk_deg, code.chk_var), np.arange(code.M)):
        for b in range(L.shape[0]):
            r, o, it = od.decode(L[b])
            out, conv, iters, post, _ = lr.decode(od, gf.mul, L[b], layer_of, 1)
            assert (conv, iters) == (r, it) and np.array_equal(out, o), b
            assert np.array_equal(post, od.state()[0]), b
            flags.append(r)
    assert 0 < sum(flags) < len(flags)


def test_schedules_differ_after_three_iterations(oracle, gf16):
    """c2v after three full iterations differs between each pair of: flooding, greedy layers, one layer per check -- otherwise the
    GPU tests could not tell the schedules apart.  (Fixed iterations, so that all three run three of them on every frame.)
    On this code the greedy assignment is four blocks of four consecutive checks, so one layer per check in ASCENDING check order
    visits the checks in an order that differs from the greedy one only inside layers -- the same schedule by definition, and the
    same c2v bit for bit (asserted: the order inside a layer is immaterial).  The one-layer-per-check assignment that is told apart
    here is therefore the one in descending check order."""
    code, ocode, gf, L = gf16
    od = oracle.Decoder(ocode, gf, oracle.EMS, 3, oracle.CANONICAL, ems_nm=8, ems_nc=3, fixed_iters=1)
    greedy = lr.greedy_layers(code.chk_deg, code.chk_var)
    assert np.array_equal(greedy, np.arange(code.M) // 4)
    for b in (0, 2, 3):
        od.decode(L[b])
        flood = od.state()[2]
        lay = lr.decode(od, gf.mul, L[b], greedy, 3, fixed_iters=1)[4]
        ser = lr.decode(od, gf.mul, L[b], np.arange(code.M)[::-1], 3, fixed_iters=1)[4]
        assert flood.shape == lay.shape == ser.shape
        assert not np.array_equal(flood, lay) and not np.array_equal(flood, ser) and not np.array_equal(lay, ser), b
        assert np.all(np.isfinite(lay)) and np.all(np.isfinite(ser))
        assert np.array_equal(lr.decode(od, gf.mul, L[b], np.arange(code.M), 3, fixed_iters=1)[4], lay), b
    # one layer holding every check would be flooding -- and is no valid assignment on a connected graph
    assert not lr.layers_valid(code.chk_deg, code.chk_var, np.zeros(code.M, dtype=np.int32))
