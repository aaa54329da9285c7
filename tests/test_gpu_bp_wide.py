"""Exact log-QSPA on codes with checks above degree 8 on a real MI355X (nbl_create_bp_wide; nbl_cn_bp_wide.hip, the programme of
nbl_cn_bp_wide_core.h) against the FP64 restatement (tests/bp_wide_cases.py), flooding and layered.  The parity statement is the
method's own (tests/test_gpu_parity.py, tests/test_gpu_layered_bp.py): out_sym, converged and iters equal; post, c2v and v2c finite and
within LLR_TOL = 1e-9 of max(1, the largest magnitude of the compared array).  Decision equality is meaningful on these inputs:
tests/test_bp_wide.py asserts that no decision of any case used here is closer than 1e-6 to going the other way.  Under flooding with
early exit the v2c of a frame that converged after iteration 1 is not compared: the kernels run the variable-node pass before the
syndrome, the reference after it, and nbl_read_state promises no v2c there.

On every code both layouts can run -- the general programme of nbl_cn_bp_core.h (debug switch 1) and the wide one (switch 3) -- they
must give the same bits: every output's sum runs over x in the same order whatever thread owns it.

Largest deviation from the restatement over all cases, one run on one MI355X: 2.84e-13 of the largest magnitude (`gf64`, flooding, the frame of wide vectors; tolerance 1e-9)."""
import numpy as np
import pytest

import nbldpc_amd as nb
import bp_wide_cases as bc
import soft_ref
from degree_util import degree_code
from test_gpu_parity import LLR_TOL, _force_generic
from test_layered_bp import _frames, case

pytestmark = pytest.mark.gpu


def close_to(dec, got, ref, tag, B=None, flooding_early=False, index=None):
    """every output of frames 0 .. B-1 of the last decode equal to the restatement's, the message state finite and within LLR_TOL;
    index[b]: the reference frame of codeword b (default b).  Returns the largest deviation seen, relative to max(1, largest magnitude)."""
    out, conv, its = got
    worst = 0.0
    for b in range(len(ref) if B is None else B):
        r = ref[b if index is None else index[b]]
        assert (conv[b], its[b]) == (r[1], r[2]), (tag, b, conv[b], its[b], r[1], r[2])
        assert np.array_equal(out[b], r[0]), (tag, b)
        post, v2c, c2v = dec.read_state(b)
        for what, a, x in (("post", post, r[3]), ("c2v", c2v, r[4]), ("v2c", v2c, r[5])):
            assert np.all(np.isfinite(a)), (tag, b, what)
            if what == "v2c" and flooding_early and r[1] and r[2] > 1:
                continue
            dev = np.max(np.abs(a - x)) / max(1.0, np.max(np.abs(x)))
            worst = max(worst, dev)
            print(tag, b, what, "deviation / largest magnitude:", dev)
            assert dev <= LLR_TOL, (tag, b, what, dev)
    print(tag, "largest deviation / largest magnitude:", worst)
    return worst


def wide_decoder(name, which, **extra):
    code, L, iters = bc.wide_case(name)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", bp_wide=True, **extra)
    dec.record_state(True)
    if which != "flooding":
        assert np.array_equal(dec.layers, bc.layer_of(name, which))
    else:
        assert dec.layers is None
    return dec, L


@pytest.mark.parametrize("which", bc.SCHEDULES)
@pytest.mark.parametrize("name", bc.NAMES)
def test_parity_with_the_restatement(oracle, name, which):
    """Check degrees 9 .. 32 over GF(4) .. GF(256): one, two and four waves per check, idle lanes below GF(64); normal, wide
    (mantissa / exponent path) and mixed frames; degree 2 and the degrees 8 / 9 beside 31 / 32 with variables of degree 1 and 8; the
    opt-in above 64 KB of LDS at GF(256), degree 32 (76,032 B); a rate-7/8 code whose frames converge at different iterations and never."""
    code = bc.wide_case(name)[0]
    assert code.chk_deg.max() > 8
    dec, L = wide_decoder(name, which)
    close_to(dec, dec.decode(L), bc.wide_reference(name, which), (name, which), flooding_early=which == "flooding")
    if name == bc.RING:
        _, (n_vn, n_syn, n_cn) = dec.last_timing()
        assert n_syn == 8 and n_cn == 8 * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    dec.close()


@pytest.mark.parametrize("which", bc.SCHEDULES)
def test_ring_fixed_iterations(oracle, which):
    """fixed_iters = 1: every frame runs 8 iterations, its outputs frozen at the first zero syndrome; the whole state is compared."""
    fixed, early = bc.wide_reference(bc.RING, which, 1), bc.wide_reference(bc.RING, which)
    for r, e in zip(fixed, early):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[4], e[4])       # (a frame that converged early went on iterating)
    dec, L = wide_decoder(bc.RING, which, fixed_iters=1)
    close_to(dec, dec.decode(L), fixed, ("fixed", which))
    dec.close()


@pytest.mark.parametrize("which", bc.SCHEDULES)
def test_ring_polling_every_iteration_and_batches(oracle, which):
    """poll_every = 1: converged codewords leave through done[b] (and the active list) beside ones that stay.  A batch of 9 codewords
    built from the case's frames repeated: each row equals its single-frame decode, and so does every prefix of the batch."""
    ref = bc.wide_reference(bc.RING, which)
    flood = which == "flooding"
    assert any(r[1] and r[2] < 8 for r in ref) and any(not r[1] for r in ref)
    dec, L = wide_decoder(bc.RING, which, poll_every=1)
    close_to(dec, dec.decode(L), ref, ("poll", which), flooding_early=flood)
    dec.close()
    dec, L = wide_decoder(bc.RING, which)
    F = L.shape[0]
    LB = bc.batch(bc.RING)
    index = np.arange(bc.B_BATCH) % F
    whole = dec.decode(LB)
    close_to(dec, whole, ref, ("B", bc.B_BATCH, which), B=bc.B_BATCH, flooding_early=flood, index=index)
    state = [dec.read_state(b) for b in range(bc.B_BATCH)]
    for b in range(F, bc.B_BATCH):                           # a repeated frame: the same bits as its first occurrence
        assert all(np.array_equal(x[b], x[b - F]) for x in whole)
        assert all(np.array_equal(x, y) for x, y in zip(state[b], state[b - F])), b
    for B in (1, 5):
        part = dec.decode(LB[:B])
        for x, y in zip(part, whole):
            assert np.array_equal(x, y[:B]), B
        for b in range(B):
            assert all(np.array_equal(x, y) for x, y in zip(dec.read_state(b), state[b])), (B, b)
    dec.close()


def _small_codes():
    """degree <= 8: the (2,4) ring codes over GF(256) and GF(64) with narrow, wide and mixed frames, a [2,3,8]-degree graph over GF(16),
    and the `all` profile over GF(4), whose checks leave a wave partly idle"""
    yield ("ring256",) + case("ring256")
    yield ("ring64",) + case("ring64")
    code = degree_code(16, 96, [2, 3, 8], [2, 3], 9)[0]
    yield "gf16-dc238", code, _frames(np.random.default_rng(16), code.N, 16, "nwm"), 3
    yield ("all-4",) + case("all-4")


@pytest.mark.parametrize("which", bc.SCHEDULES)
def test_two_layouts_one_answer(which):
    """bp_wide (switch 3) equals the general programme (switch 1: bp, or bp_layered) bit for bit on out, flags, iters, post, c2v and
    v2c.  A difference means one output's sum does not run over x in the order of lse_conv."""
    for name, code, L, iters in _small_codes():
        assert code.chk_deg.max() <= 8
        dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=None if which == "flooding" else "greedy", bp_wide=True)
        dec.record_state(True)
        runs = []
        for force in (1, 3):
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
                assert np.all(np.isfinite(x)) and np.array_equal(x, y), (name, which, f, what, float(np.max(np.abs(x - y))))
        assert tuple(a[4]) == tuple(b[4]), (a[4], b[4])


@pytest.mark.parametrize("which", bc.SCHEDULES)
def test_device_buffers_bit_llr_input_and_soft_output(which):
    """On the rate-7/8 ring code: decode_device equals decode; decode_bits equals decode on the expanded LLRs; the symbol LLRs of
    nbl_soft_output (max-log), plain and extrinsic, are bit for bit the sum formed from this decoder's own c2v (nbl_read_state) in the
    header's order -- the c2v regions hold final values, not forward partials, when the decode returns."""
    import torch
    code = bc.wide_case(bc.RING)[0]
    p = code.q.bit_length() - 1
    sigma = 0.5
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    dec = nb.Decoder(code, nb.METHOD_BP, 4, layers=None if which == "flooding" else "greedy", bp_wide=True)
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
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, b in zip(want, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    for b in range(B):                                       # the same kernels on the same numbers: bit for bit
        for a, x in zip(dec.read_state(b), state[b]):
            assert np.array_equal(a, x), b
    dec.close()
