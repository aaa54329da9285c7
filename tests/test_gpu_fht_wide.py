"""FHT sum-product decoding on codes with checks above degree 8 on a real MI355X (nbl_create_fht; nbl_cn_fht_wide.hip, the programme of
nbl_cn_fht_wide_core.h) against the numpy restatement (tests/fht_ref.py through tests/fht_wide_cases.py), flooding and layered.  The
parity statement, close_to() and the factor 16 are those of tests/test_gpu_fht.py.  On every code both layouts can run -- the register
programme of nbl_cn_fht_core.h and the wide one, selected by nbl_debug_force_generic(dec, 3) -- they must give the same bits: the
operations and their order are the header's in both.  Every case is a few frames of at most 96 symbols."""
import numpy as np
import pytest

import nbldpc_amd as nb
import fht_wide_cases as wc
import soft_ref
from test_fht import fht_case
from test_gpu_fht import close_to
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def wide_decoder(name, which, **extra):
    code, L, iters = wc.wide_case(name)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", fht=True, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, wc.layer_of(name, which))
    return dec, L


@pytest.mark.parametrize("which", wc.SCHEDULES)
@pytest.mark.parametrize("name", wc.NAMES)
def test_parity_with_the_restatement(oracle, name, which):
    """out_sym, converged and iters equal the restatement's; post, c2v and v2c within 16 x D80 in the probability domain.  Check degrees
    9 .. 32 over GF(4) .. GF(256) (one, two and four symbols per lane; idle lanes below GF(64)), normal, saturating and mixed frames;
    degree 2 and the degrees 8 / 9 beside 31 / 32 with variables of degree 1 and 8; a rate-7/8 code whose frames converge at different
    iterations and never."""
    code = wc.wide_case(name)[0]
    assert code.chk_deg.max() > 8
    dec, L = wide_decoder(name, which)
    worst = close_to(dec, dec.decode(L), wc.wide_reference(name, which), wc.tolerance(name, which), (name, which))
    print(name, which, "largest deviation", worst, "D80", wc.D80[(name, which)], "ratio", worst / wc.D80[(name, which)])
    dec.close()


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_ring_iterations_launches_fixed_mode_polling_and_batches(oracle, which):
    ref = wc.wide_reference(wc.RING, which)
    tol = wc.tolerance(wc.RING, which)
    want = wc.RING_ITERS[which]
    assert [(r[1], r[2]) for r in ref] == [(1, i) if i else (0, 8) for i in want]
    dec, L = wide_decoder(wc.RING, which)
    out, conv, its = dec.decode(L)
    assert its.tolist() == [i or 8 for i in want] and conv.tolist() == [int(i > 0) for i in want]
    close_to(dec, (out, conv, its), ref, tol, (wc.RING, which))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 8 and n_cn == 8 * (1 if which == "flooding" else wc.RING_LAYERS)
    for B in (1, 5):
        close_to(dec, dec.decode(L[:B]), ref, tol, ("B", B, which), B=B)
    dec.close()
    for poll in (1, 3):
        dec, _ = wide_decoder(wc.RING, which, poll_every=poll)
        close_to(dec, dec.decode(L), ref, tol, ("poll", poll, which))
        dec.close()
    # fixed_iters = 1: every frame runs 8 iterations, its outputs frozen at the first zero syndrome
    fixed = wc.wide_reference(wc.RING, which, 1)
    for r, e in zip(fixed, ref):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[5], e[5])
    dec, _ = wide_decoder(wc.RING, which, fixed_iters=1)
    close_to(dec, dec.decode(L), fixed, wc.tolerance(wc.RING, which, 1), ("fixed", which))
    dec.close()


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_ring_device_buffers_equal_host_buffers(oracle, which):
    import torch
    ref = wc.wide_reference(wc.RING, which)
    dec, L = wide_decoder(wc.RING, which)
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, dec.code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    close_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, wc.tolerance(wc.RING, which), ("device", which))
    state = [dec.read_state(b) for b in range(B)]
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    for b in range(B):                                  # the same kernels on the same numbers: bit for bit
        for a, x in zip(dec.read_state(b), state[b]):
            assert np.array_equal(a, x), b
    dec.close()


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_ring_bit_llr_input_and_soft_output(which):
    """decode_bits equals decode on the expanded LLRs; the symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit the sum
    formed from this decoder's own c2v (nbl_read_state) in the header's order -- the c2v regions hold final values, not forward
    products, when the decode returns."""
    code = wc.wide_case(wc.RING)[0]
    p = code.q.bit_length() - 1
    sigma = 0.5
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    dec = nb.Decoder(code, nb.METHOD_BP, 4, layers=None if which == "flooding" else "greedy", fht=True)
    dec.record_state(True)
    want = dec.decode(L)
    state = [dec.read_state(b) for b in range(4)]
    got = dec.decode_bits(lam)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)

    class G:
        N, voff = code.N, np.concatenate([[0], np.cumsum(code.var_deg)])
    sym, _ = dec.soft_output("maxlog")
    ext, _ = dec.soft_output("maxlog", extrinsic=True)
    for b in range(4):
        post, v2c, c2v = dec.read_state(b)
        for a, x in zip((post, v2c, c2v), state[b]):
            assert np.array_equal(a, x), b
        assert c2v.any() or want[2][b] == 1
        assert soft_ref.bits_equal(sym[b], soft_ref.posterior(L[b], c2v, G)), b
        assert soft_ref.bits_equal(ext[b], soft_ref.posterior(np.zeros_like(L[b]), c2v, G)), b
    assert any(want[2][b] > 1 for b in range(4))
    dec.close()


@pytest.mark.parametrize("which", wc.SCHEDULES)
@pytest.mark.parametrize("name", ["gf16", "ring256", "ring64", "all-16", "rand128"])
def test_two_layouts_one_answer(name, which):
    """Cases of tests/test_fht.py (check degrees 2 .. 8): the decoder as created runs the register programme, after
    nbl_debug_force_generic(dec, 3) the wide one.  Outputs and the whole message state are equal bit for bit, and so are the launch
    counts.  A difference means the operation order of one of them is not the header's."""
    code, L, iters = fht_case(name)
    assert code.chk_deg.max() <= 8
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", fht=True)
    dec.record_state(True)
    runs = []
    for force in (0, 3):
        _force_generic(dec, force)
        out, conv, its = dec.decode(L)
        runs.append((out.copy(), conv.copy(), its.copy(), [dec.read_state(b) for b in range(L.shape[0])], dec.last_timing()[1]))
    _force_generic(dec, 0)
    dec.close()
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, which)
    assert any(s[2].any() for s in a[3]), "no check node ran"
    for f, (sa, sb) in enumerate(zip(a[3], b[3])):
        for what, x, y in zip(("post", "v2c", "c2v"), sa, sb):
            assert np.array_equal(x, y), (name, which, f, what, float(np.max(np.abs(x - y))))
    assert tuple(a[4]) == tuple(b[4]), (a[4], b[4])


@pytest.mark.parametrize("which", wc.SCHEDULES)
def test_without_state_recording_and_with_a_growing_workspace(oracle, which):
    """wide-256 with record_state off and max_batch = 1 below the batch of 3 (the workspace grows at the first decode), then one frame
    alone: the outputs are those of the restatement."""
    code, L, iters = wc.wide_case("wide-256")
    ref = wc.wide_reference("wide-256", which)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", fht=True, max_batch=1)
    for frames in (L, L[1:2]):
        out, conv, its = dec.decode(frames)
        want = ref if frames is L else ref[1:2]
        for b, r in enumerate(want):
            assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, b)
    dec.close()
