"""Single-precision FHT decoding on codes with checks above degree 8 on a real MI355X (nbl_create_fht32_wide; nbl_cn_fht32_wide.hip, the
programme of nbl_cn_fht32_wide_core.h) against the scaled float32 restatement (tests/fht32_wide_ref.py through
tests/fht32_wide_cases.py), flooding and layered.  The parity statement is that of tests/test_gpu_fht32.py with close_to() of
tests/test_gpu_fht.py: out_sym, converged and iters equal; post, c2v and v2c compared as w(x) = exp(x - max x) within 16 x the case's
recorded D32W.  Decision equality is meaningful on these inputs: tests/test_fht32_wide.py asserts the margin of every decision of
every case.  The wide programme and the register programme of nbl_cn_fht32_core.h are NOT bit-identical on a code both run (the
scale changes how log rounds): each is held to its own restatement.  Every case is a few frames of at most 96 symbols."""
import numpy as np
import pytest

import demod_general as dg
import fht32_wide_cases as cs
import fht32_wide_ref as fw
import fht_ref as fr
import idd_kinds_cases as kc
import idd_ref as ir
import nbldpc_amd as nb
import soft_ref
from test_gpu_fht import close_to
from test_gpu_fht32 import exactly_float32
from test_gpu_idd import same
from test_gpu_idd_kinds import chain
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def wide_decoder(name, which, **extra):
    code, L, iters = cs.case(name)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", fht32_wide=True, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, cs.layer_of(name, which))
    return dec, L


@pytest.mark.parametrize("which", cs.SCHEDULES)
@pytest.mark.parametrize("name", cs.NAMES)
def test_parity_with_the_scaled_restatement(oracle, name, which):
    """out_sym, converged and iters equal the restatement's; post, c2v and v2c within 16 x D32W in the probability domain.  Check degrees
    9 .. 32 over GF(4) .. GF(256) (one, two and four symbols per lane; idle lanes below GF(64)), normal, saturating and mixed frames;
    degree 2 and the degrees 8 / 9 beside 31 / 32 with variables of degree 1 and 8; a rate-7/8 code whose frames converge at different
    iterations and never.  flat-256 is the test of step 3a: a third of the variables carry the all-zero channel vector, 16 of them at
    one degree-32 check, where the unscaled update overflows (tests/test_fht32_wide.py); every output must be finite."""
    code = cs.case(name)[0]
    assert code.chk_deg.max() > 8
    dec, L = wide_decoder(name, which)
    got = dec.decode(L)
    if name == cs.FLAT:
        assert not L[:, cs.flat_set()].any()
        for b in range(L.shape[0]):
            assert all(np.all(np.isfinite(a)) for a in dec.read_state(b)), b
    worst = close_to(dec, got, cs.reference(name, which), cs.tolerance(name, which), (name, which))
    print(name, which, "largest deviation", worst, "D32W", fw.D32W[(name, which)], "worst / D32W", worst / fw.D32W[(name, which)])
    exactly_float32(dec, L.shape[0])
    dec.close()


@pytest.mark.parametrize("which", cs.SCHEDULES)
def test_ring_iterations_launches_fixed_mode_polling_and_batches(oracle, which):
    ref = cs.reference(cs.RING, which)
    tol = cs.tolerance(cs.RING, which)
    want = cs.RING_ITERS[which]
    assert [(r[1], r[2]) for r in ref] == [(1, i) if i else (0, 8) for i in want]
    dec, L = wide_decoder(cs.RING, which)
    out, conv, its = dec.decode(L)
    assert its.tolist() == [i or 8 for i in want] and conv.tolist() == [int(i > 0) for i in want]
    close_to(dec, (out, conv, its), ref, tol, (cs.RING, which))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 8 and n_cn == 8 * (1 if which == "flooding" else cs.RING_LAYERS)
    for B in (1, 5):
        close_to(dec, dec.decode(L[:B]), ref, tol, ("B", B, which), B=B)
    dec.close()
    for poll in (1, 3):
        dec, _ = wide_decoder(cs.RING, which, poll_every=poll)
        close_to(dec, dec.decode(L), ref, tol, ("poll", poll, which))
        dec.close()
    # fixed_iters = 1: every frame runs 8 iterations, its outputs frozen at the first zero syndrome
    fixed = cs.reference(cs.RING, which, 1)
    for r, e in zip(fixed, ref):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[5], e[5])
    dec, _ = wide_decoder(cs.RING, which, fixed_iters=1)
    close_to(dec, dec.decode(L), fixed, cs.tolerance(cs.RING, which, 1), ("fixed", which))
    dec.close()
    # max_batch = 1 below the batch of 6 (the workspace grows at the first decode), state recording off, then one frame alone
    code, _, iters = cs.case(cs.RING)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", fht32_wide=True, max_batch=1)
    for frames, rows in ((L, ref), (L[1:2], ref[1:2])):
        out, conv, its = dec.decode(frames)
        for b, r in enumerate(rows):
            assert (conv[b], its[b]) == (r[1], r[2]) and np.array_equal(out[b], r[0]), (which, b)
    dec.close()


@pytest.mark.parametrize("which", cs.SCHEDULES)
def test_ring_device_buffers_equal_host_buffers(oracle, which):
    import torch
    ref = cs.reference(cs.RING, which)
    dec, L = wide_decoder(cs.RING, which)
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, dec.code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    close_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, cs.tolerance(cs.RING, which), ("device", which))
    state = [dec.read_state(b) for b in range(B)]
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    for b in range(B):                                  # the same kernels on the same numbers: bit for bit
        for a, x in zip(dec.read_state(b), state[b]):
            assert np.array_equal(a, x), b
    dec.close()


@pytest.mark.parametrize("which", cs.SCHEDULES)
def test_ring_bit_llr_input_and_soft_output(which):
    """decode_bits equals decode on the expanded LLRs; the symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit the
    header's sum of the caller's FP64 L_ch and this decoder's own c2v (nbl_read_state: the exact widening of the float c2v), in double --
    the c2v regions hold final values, not forward products, when the decode returns."""
    code = cs.case(cs.RING)[0]
    p = code.q.bit_length() - 1
    sigma = 0.5
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    assert not np.array_equal(L, L.astype(np.float32).astype(np.float64))      # (the sum below is on the FP64 L_ch, not on Lf)
    dec = nb.Decoder(code, nb.METHOD_BP, 4, layers=None if which == "flooding" else "greedy", fht32_wide=True)
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
    assert any(want[2][b] > 1 for b in range(4))
    exactly_float32(dec, 4)
    dec.close()


@pytest.mark.parametrize("which", cs.SCHEDULES)
@pytest.mark.parametrize("name", cs.SW3)
def test_two_programmes_on_one_code(oracle, name, which):
    """Cases of tests/test_fht32.py (check degrees 2 .. 8).  As created, an nbl_create_fht32_wide decoder is the decoder nbl_create_fht32
    makes: the plan is fht32 and the outputs and the whole state equal an fht32=True decoder's bit for bit.  After
    nbl_debug_force_generic(dec, 3) it runs the wide programme, with the same launch counts.  Decisions, flags and iteration counts of the
    two are equal; each is within its own tolerance of its own restatement (the unscaled one, 16 x D32R; the scaled one, 16 x D32W)."""
    case = "sw3:" + name
    code, L, iters = cs.case(case)
    assert code.chk_deg.max() <= 8
    layers = None if which == "flooding" else "greedy"
    assert nb.binding.debug_plan(code, nb.METHOD_BP, fht32_wide=True, layers=layers)[0] == ("fht32" if layers is None else "fht32_layered")
    assert nb.binding.debug_plan(code, nb.METHOD_BP, fht32_wide=True, layers=layers, force_generic=3)[0] == ("fht32_wide" if layers is None else "fht32_wide_layered")
    plain = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht32=True)
    plain.record_state(True)
    want = plain.decode(L)
    want_state = [plain.read_state(b) for b in range(L.shape[0])]
    plain.close()
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht32_wide=True)
    dec.record_state(True)
    runs = []
    for force, ref, tol in ((0, cs.register_reference(case, which), 16.0 * cs.D32R[(case, which)]), (3, cs.reference(case, which), cs.tolerance(case, which))):
        _force_generic(dec, force)
        got = dec.decode(L)
        close_to(dec, got, ref, tol, (case, which, "switch", force))
        runs.append((got[0].copy(), got[1].copy(), got[2].copy(), [dec.read_state(b) for b in range(L.shape[0])], dec.last_timing()[1]))
        exactly_float32(dec, L.shape[0])
    _force_generic(dec, 0)
    dec.close()
    a, b = runs
    for k in range(3):                                   # as created: bit for bit the fht32=True decoder
        assert np.array_equal(a[k], want[k]), (case, which, k)
    for f, (sa, sw) in enumerate(zip(a[3], want_state)):
        for what, x, y in zip(("post", "v2c", "c2v"), sa, sw):
            assert np.array_equal(x, y), (case, which, f, what)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (case, which)
    assert any(s[2].any() for s in b[3]), "no check node ran"
    assert tuple(a[4]) == tuple(b[4]), (a[4], b[4])
    diff = max(fr.w_dev(x, y) for sa, sb in zip(a[3], b[3]) for x, y in zip(sa, sb))
    print(case, which, "largest difference between the two programmes in the probability domain:", diff)


@pytest.mark.parametrize("which", cs.SCHEDULES)
def test_iterative_demapping_is_the_chain_of_public_calls(which):
    """decode_samples_idd with 3 passes on the wide64 graph of tests/idd_kinds_cases.py (check degrees 9 .. 32 over GF(64), interleaved
    16-QAM, the noise of its FP64 FHT cells) equals the loop written out with public calls."""
    sigma = 0.175 if which == "flooding" else 0.185
    sh = kc.shape("wide64")
    rx = ir.loop_samples(sh, sigma, 24)
    dec = nb.Decoder(kc.graph("wide64")[0], nb.METHOD_BP, 3, layers=None if which == "flooding" else "greedy", fht32_wide=True)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
    want = chain(dec, rx, sigma, 3)
    got = dec.decode_samples_idd(rx, sigma, 3, "maxlog")
    cnt = kc.counts(got[1], got[3])
    print("wide64", which, "pass 1 / later / never =", cnt)
    same(got, want, ("wide64", which))
    assert cnt[0] >= 1 and cnt[1] + cnt[2] >= 2, cnt     # the chain went beyond pass 1
    dec.close()
