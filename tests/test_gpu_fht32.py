"""Single-precision FHT sum-product decoding on a real MI355X (nbl_create_fht32; nbl_cn_fht32.hip, nbl_fht32.hip) against its float32
numpy restatement (tests/fht32_ref.py), flooding and layered.  The parity statement is the method's own (include/nbldpc.h): out_sym,
converged and iters equal; post, c2v and v2c compared as w(x) = exp(x - max x) within 16 x the case's recorded D32, the deviation
between the restatement with numpy's float32 exp / log and with exp / log taken in float64 and rounded once.  The GPU evaluates the
same float32 adds and products and differs only in expf / logf: 4 x for a 2-ulp device function against a correctly rounded one, 4 x
for the sample-to-sample spread.  Decision equality is meaningful on these inputs: tests/test_fht32.py asserts that every decision of
every case has a margin of 64 x what the two evaluations differ by.  Shapes are those of tests/test_gpu_fht.py."""
import numpy as np
import pytest

import demod_general as dg
import idd_ref as ir
import nbldpc_amd as nb
import soft_ref
from test_fht32 import degree9_code, fht32_case, fht32_reference, tolerance
from test_gpu_fht import close_to
from test_gpu_idd import same
from test_gpu_idd_kinds import chain
from test_gpu_layered import assignments

pytestmark = pytest.mark.gpu

SCHEDULES = ("flooding", "greedy")


def fht32_decoder(name, which="flooding", **extra):
    code, L, iters = fht32_case(name)
    layers = None if which == "flooding" else "greedy" if which == "greedy" else assignments(code)[which]
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht32=True, **extra)
    dec.record_state(True)
    return dec, L


def exactly_float32(dec, B):
    """every double nbl_read_state returns is finite and exactly representable in binary32"""
    for b in range(B):
        for what, a in zip(("post", "v2c", "c2v"), dec.read_state(b)):
            assert np.all(np.isfinite(a)) and np.array_equal(a, a.astype(np.float32).astype(np.float64)), (b, what)


@pytest.mark.parametrize("which", SCHEDULES)
def test_gf16_frames_that_converge_at_different_iterations(oracle, which):
    """Shipped GF(16) code, 8 frames at 1.5 dB, 8 iterations: frames converge at different iterations and never; iters is checked per
    frame.  Launches per iteration as nbl_last_timing counts them: variable-node pass (or decision), syndrome, one check-node launch (or
    one per layer).  The narrowing launch of the call has no counter there (it follows the init launch and is timed with it, in the
    total ms[3] alone), so the three counts are those of the FP64 kind."""
    ref = fht32_reference("gf16", which)
    dec, L = fht32_decoder("gf16", which)
    dec.profiling(True)
    close_to(dec, dec.decode(L), ref, tolerance("gf16", which), ("gf16", which))
    ms, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 8 and n_cn == 8 * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    assert ms[3] >= ms[0] + ms[1] + ms[2] > 0.0
    assert (dec.layers is None) == (which == "flooding")
    exactly_float32(dec, L.shape[0])
    dec.close()


@pytest.mark.parametrize("which", ["flooding", "greedy", "serial", "other"])
@pytest.mark.parametrize("name", ["ring256", "ring64"])
def test_ring_codes_normal_saturating_and_mixed(oracle, name, which):
    """_ring_code(256, 8, 4) (four symbols per lane) and _ring_code(64, 8, 4) (one): 3 frames -- normal(-2, 4), normal(-900, 700) (every
    vector one-hot, the outputs at the floor), narrow and wide vectors mixed in one check -- 3 iterations, flooding and under the three
    assignments."""
    dec, L = fht32_decoder(name, which)
    close_to(dec, dec.decode(L), fht32_reference(name, which), tolerance(name, which), (name, which))
    if which != "flooding":
        assert np.array_equal(dec.layers, assignments(fht32_case(name)[0])[which])
    exactly_float32(dec, L.shape[0])
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
@pytest.mark.parametrize("name", ["all-4", "all-8", "all-16", "dv48-32", "rand128"])
def test_degrees_and_fields(oracle, name, which):
    """The `all` degree profile (checks of degree 2-8, variables of degree 1-8) over GF(4), GF(8), GF(16): lanes idle at q < 64;
    variables of degree 4-8 over GF(32); an irregular graph over GF(128) (two symbols per lane).  One real-valued frame."""
    code = fht32_case(name)[0]
    if name.startswith("all"):
        assert code.var_deg.min() == 1 and code.var_deg.max() == 8 and (code.chk_deg.min(), code.chk_deg.max()) == (2, 8)
    dec, L = fht32_decoder(name, which)
    close_to(dec, dec.decode(L), fht32_reference(name, which), tolerance(name, which), (name, which))
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_fixed_iterations(oracle, which):
    """fixed_iters = 1: every frame runs max_iter iterations, its outputs frozen at the first zero syndrome, its state that of
    iteration 8; against the restatement's fixed mode."""
    ref, early = fht32_reference("gf16", which, 1), fht32_reference("gf16", which)
    assert any(r[1] and r[2] < 8 for r in ref)
    for r, e in zip(ref, early):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[5], e[5])      # (a frame that converged early went on iterating)
    dec, L = fht32_decoder("gf16", which, fixed_iters=1)
    close_to(dec, dec.decode(L), ref, tolerance("gf16", which, 1), ("fixed", which))
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_poll_every_and_batches_of_one_and_five(oracle, which):
    ref = fht32_reference("gf16", which)
    tol = tolerance("gf16", which)
    for poll in (1, 3):
        dec, L = fht32_decoder("gf16", which, poll_every=poll)
        close_to(dec, dec.decode(L), ref, tol, ("poll", poll, which))
        dec.close()
    dec, L = fht32_decoder("gf16", which)
    for B in (1, 5):
        close_to(dec, dec.decode(L[:B]), ref, tol, ("B", B, which), B=B)
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_device_buffers_equal_host_buffers(oracle, which):
    import torch
    ref = fht32_reference("gf16", which)
    dec, L = fht32_decoder("gf16", which)
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, dec.code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    close_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, tolerance("gf16", which), ("device", which))
    state = [dec.read_state(b) for b in range(B)]
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    for b in range(B):                                  # the same kernels on the same numbers: bit for bit
        for a, x in zip(dec.read_state(b), state[b]):
            assert np.array_equal(a, x), b
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_bit_llr_input_and_soft_output(oracle, which):
    """decode_bits equals decode on the expanded LLRs; the symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit the
    header's sum of the caller's FP64 L_ch and this decoder's own c2v (nbl_read_state: the exact widening of the float c2v), in double."""
    code = fht32_case("gf16")[0]
    p = code.q.bit_length() - 1
    sigma = 0.95
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    assert not np.array_equal(L, L.astype(np.float32).astype(np.float64))      # (the sum below is on the FP64 L_ch, not on Lf)
    dec = nb.Decoder(code, nb.METHOD_BP, 4, layers=None if which == "flooding" else "greedy", fht32=True)
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
        assert np.array_equal(c2v, c2v.astype(np.float32).astype(np.float64))
        assert soft_ref.bits_equal(sym[b], soft_ref.posterior(L[b], c2v, G)), b
        assert soft_ref.bits_equal(ext[b], soft_ref.posterior(np.zeros_like(L[b]), c2v, G)), b
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_iterative_demapping_is_the_chain_of_public_calls(which):
    """decode_samples_idd(passes = 2) on the general demodulator equals the loop written out with public calls -- decode_samples,
    extrinsic soft output, decode_samples with that prior on the survivors -- on one FP32 decoder per schedule.  Two layouts: the GF(16)
    code on the 4-point constellation of tests/test_gpu_idd.py (gf16_qpsk_aligned, the general kernel forced: no point carries bits of
    two symbols, so the prior moves nothing and pass 2 repeats pass 1 on the survivors), and GF(64) on interleaved 16-QAM, where it
    does (the layout and noise of the FP64 FHT cells of tests/idd_kinds_cases.py)."""
    layers = None if which == "flooding" else "greedy"
    for name, sigma, B in (("gf16_qpsk_aligned", 0.8, 16), ("gf64_16qam_interleaved", 0.4 if which == "flooding" else 0.5, 24)):
        sh = dg.shape(name)
        rx = ir.loop_samples(sh, sigma, B)               # the all-zero codeword plus noise
        dec = nb.Decoder(dg.graph(name)[0], nb.METHOD_BP, 3, layers=layers, fht32=True)
        dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG, force_general=True)
        want = chain(dec, rx, sigma, 2)
        got = dec.decode_samples_idd(rx, sigma, 2, "maxlog")
        print(name, which, "converged", got[1].tolist(), "passes", got[3].tolist())
        same(got, want, (name, which))
        assert (got[3] == 2).any(), got[3]               # the loop went beyond pass 1
        dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_workspace_is_smaller_until_the_state_is_read(which):
    """nbl_workspace_bytes of a fresh FP32 decoder is below that of an nbl_create_fht decoder of the same code and max_batch (float
    messages, and no FP64 copy of them); the FP64 c2v / v2c come with the first nbl_read_state."""
    code, L, iters = fht32_case("gf16")
    layers = None if which == "flooding" else "greedy"
    d32 = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht32=True, max_batch=8)
    d64 = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht=True, max_batch=8)
    fresh = d32.workspace_bytes()
    E, q = int(code.var_deg.sum()), code.q
    assert 0 < fresh < d64.workspace_bytes(), (fresh, d64.workspace_bytes())
    d32.decode(L)
    assert d32.workspace_bytes() == fresh
    d32.read_state(0, post=False)
    assert d32.workspace_bytes() == fresh + 2 * 8 * E * q * 8    # c2v and v2c [8][E][q] doubles
    d32.close()
    d64.close()


def test_a_degree_nine_check_is_refused_and_decodes_in_double_precision():
    code = degree9_code()
    with pytest.raises(nb.NblError) as e:
        nb.Decoder(code, nb.METHOD_BP, 3, fht32=True)
    assert e.value.status == -1 and "nbl_create_fht32" in str(e.value) and "check degree 9 " in str(e.value) and "nbl_create_fht " in str(e.value)
    dec = nb.Decoder(code, nb.METHOD_BP, 3, fht=True)
    L = np.random.default_rng(3209).normal(-2, 4, (2, code.N, code.q - 1))
    out, conv, its = dec.decode(L)
    assert out.shape == (2, code.N) and ((its >= 1) & (its <= 3)).all()
    dec.close()
