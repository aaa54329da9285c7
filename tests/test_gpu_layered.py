"""The layered (check-serial) EMS schedule on a real MI355X (nbl_create_layered, nbl_cn_layered.hip) against its numpy restatement
(tests/layered_ref.py, which takes the per-check update from the reference-pinned oracle): out_sym, converged, iters, post and c2v of
every frame, bit for bit.  Shapes are the smallest that reach each code path: the shipped GF(16) code, ring graphs over GF(64) and
GF(256) (one and four symbols per lane), the `all` degree profile (checks 2-8, variables 1-8) over GF(4), GF(8) and GF(32)."""
import functools

import numpy as np
import pytest

import nbldpc_amd as nb
import layered_ref as lr
import pyoracle
from degree_util import profile_code
from test_abi import _ring_code
from test_gpu_parity import _bpsk_llr_zero, _force_generic
from test_layered import GF16, oracle_edges

pytestmark = pytest.mark.gpu


def assignments(code):
    """greedy | one layer per check | a valid assignment that is neither: the greedy layers in reverse order, the last check in a
    layer of its own behind them"""
    greedy = lr.greedy_layers(code.chk_deg, code.chk_var)
    other = greedy.max() - greedy
    other[-1] = greedy.max() + 1
    other = np.unique(other, return_inverse=True)[1].reshape(-1)   # (no gap where the last check left a layer empty)
    assert lr.layers_valid(code.chk_deg, code.chk_var, other)
    assert not np.array_equal(other, greedy) and other.max() + 1 < code.M
    return {"greedy": greedy, "serial": np.arange(code.M, dtype=np.int32), "other": other.astype(np.int32)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, kw, L, max_iter) of a named case; built once"""
    if name == "gf16":
        code = nb.Code(GF16)
        # all-zero codeword over BPSK at 2.0 dB: chosen on the CPU with the restatement alone so that some frames converge (at
        # iterations 2 .. 5) and some do not within 6 iterations; asserted on the reference's flags below
        return code, dict(ems_nm=8, ems_nc=3), _bpsk_llr_zero(np.random.default_rng(77), code, 8, 2.0), 6
    if name in ("ring256", "ring64"):
        q = int(name[4:])
        code = _ring_code(q, 8, 4)
        kw = dict(ems_nm=16, ems_nc=3) if q == 256 else dict(ems_nm=8, ems_nc=2, ems_factor=1.15, ems_offset=0.2)
        L = np.random.default_rng(q).normal(-1.5, 3.0, (4, code.N, q - 1))
        L[1, ::3] = 0.0                                 # every third symbol erased
        return code, kw, L, 4
    prof, q, nc = name.split("-")                       # all-<q>-<nc>
    q, nc = int(q), int(nc)
    code = profile_code(prof, q)[0]
    L = np.random.default_rng(10 * q + nc).normal(-1.5, 3.0, (4, code.N, q - 1))
    L[1, ::3] = 0.0
    L[2] = np.round(L[2])                               # an integer grid: exact ties (factor 1, offset 0: every sum exact)
    return code, dict(ems_nm=q // 2, ems_nc=nc), L, 4


@functools.lru_cache(maxsize=None)
def reference(name, which, fixed=0):
    """[(out, converged, iters, post, c2v)] per frame of a case under assignment `which`; computed once and shared"""
    code, kw, L, iters = case(name)
    ocode = pyoracle.Code(edges=oracle_edges(code))
    g = lr.Graph(ocode)
    assert np.array_equal(g.c_var, code.chk_var) and np.array_equal(g.c_h, code.chk_h) and np.array_equal(g.v_chk, code.var_chk)
    gf = pyoracle.GF(code.q)
    od = pyoracle.Decoder(ocode, gf, pyoracle.EMS, iters, pyoracle.CANONICAL, fixed_iters=fixed, **kw)
    return lr.decode_batch(od, gf.mul, L, assignments(code)[which], iters, fixed_iters=fixed)


def equal_to(dec, got, ref, tag, B=None):
    """every output and the message state of frames 0 .. B-1 of the last decode against the restatement"""
    out, conv, its = got
    for b in range(len(ref) if B is None else B):
        r_out, r_conv, r_its, r_post, r_c2v = ref[b]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, v2c, c2v = dec.read_state(b, v2c=False)
        assert v2c is None
        assert np.array_equal(post, r_post), (tag, b, "post")
        assert np.array_equal(c2v, r_c2v), (tag, b, "c2v")


def layered(name, which="greedy", **extra):
    code, kw, L, iters = case(name)
    dec = nb.Decoder(code, nb.METHOD_EMS, iters, layers="greedy" if which == "greedy" else assignments(code)[which], **kw, **extra)
    dec.record_state(True)
    return dec, L


def test_gf16_frames_that_converge_at_different_iterations(oracle):
    """Shipped GF(16) code, nm = 8, nc = 3, 8 frames, 6 iterations, greedy layers: some frames converge, at different iterations,
    some do not; iters is checked per frame, the state of a converged frame is what iteration iters - 1 left."""
    ref = reference("gf16", "greedy")
    flags = [r[1] for r in ref]
    assert 0 < sum(flags) < len(flags) and len({r[2] for r in ref if r[1]}) >= 3, [(r[1], r[2]) for r in ref]
    dec, L = layered("gf16")
    equal_to(dec, dec.decode(L), ref, "gf16")
    assert np.array_equal(dec.layers, assignments(case("gf16")[0])["greedy"])
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 6 and n_cn == 6 * (int(dec.layers.max()) + 1)   # launches per iteration: n_layers + decision + syndrome
    dec.close()


@pytest.mark.parametrize("which", ["greedy", "serial", "other"])
@pytest.mark.parametrize("name", ["ring256", "ring64"])
def test_ring_codes_under_three_assignments(oracle, name, which):
    """_ring_code(256, 8, 4) with nm = 16, nc = 3 and _ring_code(64, 8, 4) with nm = 8, nc = 2 (shaped: factor 1.15, offset 0.2):
    4 frames, 4 iterations, under the greedy assignment, one layer per check, and a caller's assignment that is neither.  The three
    references differ from each other, so an assignment that is not honoured cannot pass."""
    refs = {w: reference(name, w) for w in ("greedy", "serial", "other")}
    for a, b in (("greedy", "serial"), ("greedy", "other"), ("serial", "other")):
        assert any(not np.array_equal(x[4], y[4]) for x, y in zip(refs[a], refs[b])), (a, b)
    dec, L = layered(name, which)
    equal_to(dec, dec.decode(L), refs[which], (name, which))
    assert np.array_equal(dec.layers, assignments(case(name)[0])[which])
    dec.close()


@pytest.mark.parametrize("nc", [0, 3])
@pytest.mark.parametrize("q", [4, 8, 32])
def test_small_fields_on_every_degree(oracle, q, nc):
    """GF(4), GF(8), GF(32) on the `all` degree profile (checks of degree 2-8, variables of degree 1-8, degree-1 variables included:
    their input to a check is L_ch + c2v - c2v), nm = q / 2, nc = 0 (conf(q,1) alone) and 3 (deviation counting), 4 frames (one with
    erasures, one on an integer grid), 4 iterations."""
    name = f"all-{q}-{nc}"
    code = case(name)[0]
    assert code.var_deg.min() == 1 and code.var_deg.max() == 8 and (code.chk_deg.min(), code.chk_deg.max()) == (2, 8)
    dec, L = layered(name)
    equal_to(dec, dec.decode(L), reference(name, "greedy"), name)
    dec.close()


def test_batches_of_one_and_five(oracle):
    ref = reference("gf16", "greedy")
    dec, L = layered("gf16")
    for B in (1, 5):
        equal_to(dec, dec.decode(L[:B]), ref, ("B", B), B=B)
    dec.close()


def test_fixed_iterations(oracle):
    """fixed_iters = 1: every frame runs max_iter iterations, its outputs frozen at the first zero syndrome; against the
    restatement's fixed mode."""
    ref = reference("gf16", "greedy", 1)
    assert any(r[1] and r[2] < 6 for r in ref)
    dec, L = layered("gf16", fixed_iters=1)
    equal_to(dec, dec.decode(L), ref, "fixed")
    dec.close()


def test_poll_every_does_not_change_results(oracle):
    """poll_every 0, 1 and 4: identical results; with polling and 1040 frames the active list takes over after the first window
    (the grids of a layer then cover the frames still iterating)."""
    ref = reference("gf16", "greedy")
    for poll in (0, 1, 4):
        dec, L = layered("gf16", poll_every=poll)
        equal_to(dec, dec.decode(L), ref, ("poll", poll))
        if poll == 1:
            dec.record_state(False)
            big = np.concatenate([L] * 130, axis=0)
            out, conv, its = dec.decode(big)
            for b in range(big.shape[0]):
                r = ref[b % L.shape[0]]
                assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), ("active list", b)
        dec.close()


def test_device_buffers_equal_host_buffers(oracle):
    import torch
    ref = reference("gf16", "greedy")
    dec, L = layered("gf16")
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, dec.code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    equal_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, "device")
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    dec.close()


def test_layers_round_trip_and_v2c_is_refused(oracle):
    code, kw, L, iters = case("gf16")
    for which, want in assignments(code).items():
        dec = nb.Decoder(code, nb.METHOD_EMS, iters, layers=want, **kw)
        assert np.array_equal(dec.layers, want), which
        n = np.zeros(1, dtype=np.int32)
        assert dec.lib.nbl_get_layers(dec.h, None, n.ctypes.data_as(nb.binding.C.POINTER(nb.binding.C.c_int32))) == 0 and n[0] == want.max() + 1
        assert dec.lib.nbl_get_layers(dec.h, None, None) == 0
        dec.close()
    dec = nb.Decoder(code, nb.METHOD_EMS, iters, layers="greedy", **kw)
    dec.decode(L[:2])
    with pytest.raises(nb.NblError) as e:
        dec.read_state(0, post=False)                   # v2c non-NULL
    assert e.value.status == -2 and "v2c" in str(e.value)
    dec.close()
    flood = nb.Decoder(code, nb.METHOD_EMS, iters, **kw)
    assert flood.layers is None                         # NBL_ERR_ARG on a flooding decoder
    flood.close()


@pytest.mark.parametrize("name", ["gf16", "ring256", "all-32-3"])
def test_flooding_decoder_is_unchanged(oracle, name):
    """A decoder made by nbl_create on the same inputs still equals the flooding oracle in every kernel variant -- variant 1 is the
    general EMS kernel, whose check-node programme the layered kernel shares."""
    code, kw, L, iters = case(name)
    od = oracle.Decoder(oracle.Code(edges=oracle_edges(code)), oracle.GF(code.q), oracle.EMS, iters, oracle.CANONICAL, **kw)
    ref = []
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        ref.append((r, o.copy(), it, [x.copy() for x in od.state()]))
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, nb.METHOD_EMS, iters, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        for b, (r, o, it, st) in enumerate(ref):
            assert (conv[b], its[b]) == (r, it) and np.array_equal(out[b], o), (name, variant, b)
            for k, (a, x) in enumerate(zip(dec.read_state(b), st)):
                if not (k == 1 and r == 1 and it >= 2):
                    assert np.array_equal(a, x), (name, variant, b, k)
        dec.close()
