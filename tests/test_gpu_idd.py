"""Iterative demapping on a real MI355X (nbl_decode_batch_samples_prior, nbl_soft_output_ex, nbl_decode_batch_samples_idd /
nbl_decode_batch_resident_idd; nbl_demod.hip, nbl_soft.hip, nbl_idd.hip) against the numpy restatement of include/nbldpc.h's definition
(tests/idd_ref.py), which tests/test_idd.py holds against a brute force and two anchors on the CPU.

  the prior-aware demodulator kernel: the L_ch the decoder saw, max-log bit for bit, log-sum within ir.LOGSUM_TOL
  the extrinsic soft output: tests/soft_cases.py's frames and modes, against soft_ref.posterior(zeros, c2v) on the decoder's own state
      and, where one exists, on the oracle's
  the loop: every output bit for bit against idd_ref's loop on the canonical oracle under max-log metrics (tests/test_idd.py asserts
      the convergence mix of the cells); batch independence, the active list, both entry points, state hygiene, the refusals
The loop under log-sum is not pinned end to end (one rounding can flip a convergence): it is run, and one pass from a given prior
is compared."""
import numpy as np
import pytest

import demod_general as dg
import idd_ref as ir
import layered_ref as lr
import nbldpc_amd as nb
import soft_cases as sc
import soft_ref as sr
from test_gpu_parity import _force_generic
from test_gpu_soft import assert_mix

pytestmark = pytest.mark.gpu

METRICS = {"maxlog": ir.MAXLOG, "logsum": ir.LOGSUM}
SIGMA = ir.KERNEL_SIGMA


def demod_decoder(name, metric, method=nb.METHOD_BP, max_iter=1, **kw):
    sh = dg.shape(name)
    dec = nb.Decoder(dg.graph(name)[0], method, max_iter, **kw)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=metric)
    return dec


def lch(dec, B):
    return np.stack([dec.read_lch(b) for b in range(B)])


# ---- the prior-aware demodulator kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_kernel_equals_the_restatement(name, metric):
    """priors 4 randn, one row of zeros, one row of +-50"""
    sh, rx, prior = ir.kernel_case(name)
    want, scale, _ = ir.kernel_want(name, METRICS[metric])
    dec = demod_decoder(name, METRICS[metric])
    out, _, _ = dec.decode_samples(rx, SIGMA, prior=prior)
    got = lch(dec, rx.shape[0])
    err = np.abs(got - want)
    print(f"{name} {metric}: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} units of 2^-53 "
          f"(tolerance {ir.LOGSUM_TOL / 2.0 ** -53:.1f})")
    if metric == "maxlog":
        assert sr.bits_equal(got, want)
    else:
        assert (err <= ir.LOGSUM_TOL * scale).all()
    if name != "gf16_qpsk_aligned":                                           # the prior entered: not the prior-less LLRs
        assert not sr.bits_equal(got, dg.demod(sh["points"], sh["src"], rx, SIGMA, sh["N"], sh["p"], METRICS[metric])[0])
    ref, _, _ = dec.decode(got)                                               # and the decode used them
    assert np.array_equal(out, ref)
    dec.close()


@pytest.mark.parametrize("name", sorted(dg.SHAPES))
def test_zero_prior_and_no_prior(name):
    """a zero prior through the new instance, prior=None and passes=1 through the old one: the same bytes in every output, and the
    L_ch of the prior-less restatement"""
    sh, rx, prior = ir.kernel_case(name)
    dec = demod_decoder(name, ir.MAXLOG, nb.METHOD_EMS, 3, ems_nm=min(16, sh["q"] // 2), ems_nc=3)
    base = dec.decode_samples(rx, SIGMA)
    L0 = lch(dec, rx.shape[0])
    assert sr.bits_equal(L0, dg.demod(sh["points"], sh["src"], rx, SIGMA, sh["N"], sh["p"], dg.MAXLOG)[0])
    for zero in (0.0, -0.0):
        z = dec.decode_samples(rx, SIGMA, prior=np.full(prior.shape, zero))
        assert sr.bits_equal(lch(dec, rx.shape[0]), L0)
        for a, b in zip(z, base):
            assert np.array_equal(a, b)
    none = dec.decode_samples(rx, SIGMA, prior=None)
    assert dec.lib.nbl_decode_batch_samples_prior(dec.h, np.ascontiguousarray(rx).ctypes.data, None, SIGMA, rx.shape[0], none[0].ctypes.data, None, None) == 0
    one = dec.decode_samples_idd(rx, SIGMA, 1)
    assert sr.bits_equal(lch(dec, rx.shape[0]), L0)
    for a, b, c in zip(none, base, one):
        assert np.array_equal(a, b) and np.array_equal(c, b)
    assert (one[3] == 1).all()
    dec.soft_output("maxlog")                                                 # passes = 1 IS the plain call: the state is the batch's
    dec.close()


def test_forced_general_bpsk_and_qary_have_no_foreign_position():
    """the general kernel forced onto M = 2 and M = q: a random prior changes nothing, bit for bit; the specialised kernels accept a
    prior and ignore it; the loop on them stops after pass 1"""
    rng = np.random.default_rng(5)
    code = nb.Code(dg.U16)
    N, p = code.N, 4
    Lb = (N - 1) * p
    src_b = dg.src_table(N, p, (5,), 1, Lb)
    pts_b = dg.named_points("BPSK")
    rx_b = pts_b[rng.integers(0, 2, (3, Lb))] + SIGMA * rng.standard_normal((3, Lb, 2))
    code_q, _ = dg.graph("gf64_16qam")
    src_q, Lq = dg.qary_src(code_q.N, 6, (3,))
    src_sym = np.array([-1 if n == 3 else n - (n > 3) for n in range(code_q.N)], dtype=np.int32)
    pts_q = dg.named_points("GRAY_64QAM")
    rx_q = pts_q[rng.integers(0, 64, (3, Lq))] + SIGMA * rng.standard_normal((3, Lq, 2))
    for cd, M, L, src, src_own, pts, rx in ((code, 2, Lb, src_b, src_b, pts_b, rx_b), (code_q, 64, Lq, src_q, src_sym, pts_q, rx_q)):
        prior = 4 * rng.standard_normal((3, cd.N * (cd.q.bit_length() - 1)))
        dec = nb.Decoder(cd, nb.METHOD_EMS, 2, ems_nm=8, ems_nc=2)
        for forced in (True, False):
            if forced:
                dec.set_demodulator(M, L, src, pts, metric=dg.LOGSUM, force_general=True)
            else:
                dec.set_demodulator(M, L, src_own, pts)
            base = dec.decode_samples(rx, SIGMA)
            L0 = lch(dec, 3)
            got = dec.decode_samples(rx, SIGMA, prior=prior)
            assert sr.bits_equal(lch(dec, 3), L0), (M, forced)
            loop = dec.decode_samples_idd(rx, SIGMA, 3)
            for a, b, c in zip(base, got, loop):
                assert np.array_equal(a, b) and np.array_equal(a, c)
            assert np.array_equal(loop[3], np.where(base[1], 1, 3))
        dec.close()


# ---- the extrinsic soft output ------------------------------------------------------------------------------------------------------
EXT_GRID = ([(sc.U16, m, 0) for m in ("ems", "tems", "bp", "bstems", "ems_layered", "tems_layered")]
            + [(sc.U256, "ems", g) for g in (0, 1, 2)] + [("all8", "ems", 0)])


def check_extrinsic(dec, name, method, mode, L, got, tag):
    import pyoracle
    out, conv, its = got
    code, edges, _ = sc.graph(name)
    p = code.q.bit_length() - 1
    B = L.shape[0]
    g = lr.Graph(pyoracle.Code(edges=edges))
    fixed = sc.MODES[mode].get("fixed_iters", 0)
    # flags = 0 is the existing call, byte for byte
    for metric in ("maxlog", "logsum"):
        for a, b in zip(dec.soft_output(metric), dec.soft_output(metric, extrinsic=0)):
            assert sr.bits_equal(a, b), (tag, metric, "flags 0")
    sym, bits = dec.soft_output("maxlog", extrinsic=True)
    sym2, bits_ls = dec.soft_output("logsum", extrinsic=True)
    assert sym.shape == (B, code.N, code.q - 1) and bits.shape == (B, code.N * p) and sr.bits_equal(sym, sym2)
    zeros = np.zeros((code.N, code.q - 1))
    for b in range(B):                                                        # the definition on the decoder's own state
        _, _, c2v = dec.read_state(b, post=False, v2c=False)
        assert sr.bits_equal(sym[b], sr.posterior(zeros, c2v, g)), (tag, b, "definition")
    if method in sc.EXACT:                                                    # and on the oracle's
        ref = sc.oracle_state(name, method, fixed)
        for b in range(B):
            r_conv, r_its, _, r_c2v = ref[b]
            assert (conv[b], its[b]) == (r_conv, r_its), (tag, b)
            assert sr.bits_equal(sym[b], sr.posterior(zeros, r_c2v, g)), (tag, b, "oracle")
    assert sr.bits_equal(bits, sr.bit_marginals(sym, p, sr.MAXLOG)), (tag, "max-log")
    err = sr.logsum_error(bits_ls, sr.bit_marginals(sym, p, sr.LOGSUM, np.longdouble), sym)
    print(f"{tag}: extrinsic log-sum error {err:.3e} = {err * 2.0 ** 53:.2f} units of 2^-53 (tolerance {sr.LOGSUM_TOL:.3e})")
    assert err <= sr.LOGSUM_TOL, (tag, err)
    a_post, _ = dec.soft_output("maxlog", bits=False)                         # extrinsic + channel = a-posteriori, up to the order of the sum
    assert np.allclose(a_post, sym + L, rtol=0, atol=1e-9 * max(1.0, float(np.abs(a_post).max())))


@pytest.mark.parametrize("mode", sorted(sc.MODES))
@pytest.mark.parametrize("name,method,generic", EXT_GRID)
def test_extrinsic_soft_output(oracle, name, method, generic, mode):
    L = sc.frames(name)[0]
    tag = (name, method, generic, mode)
    dec = sc.decoder(name, method, mode)
    _force_generic(dec, generic)
    got = dec.decode(L)
    if not sc.MODES[mode].get("fixed_iters", 0):
        assert_mix(name, method, got[1], got[2], tag)
    check_extrinsic(dec, name, method, mode, L, got, tag)
    dec.close()


@pytest.mark.parametrize("name", [sc.U16, sc.U256])
def test_extrinsic_with_max_iter_zero_is_all_zeros(oracle, name):
    L = sc.frames(name)[0]
    dec = sc.decoder(name, "ems", "poll0", max_iter=0)
    dec.decode(L)
    sym, bits = dec.soft_output("maxlog", extrinsic=True)
    _, bits_ls = dec.soft_output("logsum", sym=False, extrinsic=True)
    for x in (sym, bits, bits_ls):
        assert sr.bits_equal(x, np.zeros_like(x))                             # +0.0, every one
    dec.close()


def test_extrinsic_device_entry_point(oracle):
    import torch
    L = sc.frames(sc.U16)[0]
    code = sc.graph(sc.U16)[0]
    B, p = L.shape[0], 4
    dec = sc.decoder(sc.U16, "ems", "poll2")
    dec.decode(L)
    h_sym, h_bits = dec.soft_output("maxlog", extrinsic=True)
    a_sym, a_bits = dec.soft_output("maxlog")
    sym = torch.zeros((B, code.N, code.q - 1), dtype=torch.float64, device="cuda")
    bits = torch.zeros((B, code.N * p), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    dec.soft_output_device("maxlog", sym.data_ptr(), bits.data_ptr(), st, extrinsic=True)
    torch.cuda.synchronize()
    assert sr.bits_equal(sym.cpu().numpy(), h_sym) and sr.bits_equal(bits.cpu().numpy(), h_bits)
    dec.soft_output_device("maxlog", sym.data_ptr(), bits.data_ptr(), st, extrinsic=0)
    torch.cuda.synchronize()
    assert sr.bits_equal(sym.cpu().numpy(), a_sym) and sr.bits_equal(bits.cpu().numpy(), a_bits)
    dec.close()


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def loop_decoder(cell, poll_every, metric=ir.MAXLOG, **kw):
    name, max_iter, _ = ir.LOOP_CELLS[cell] if cell in ir.LOOP_CELLS else ir.TEMS_CELLS[cell]
    if cell in ir.LOOP_CELLS:
        return demod_decoder(name, metric, nb.METHOD_EMS, max_iter, fixed_iters=0, poll_every=poll_every, **ir.LOOP_EMS, **kw)
    return demod_decoder(name, metric, nb.METHOD_TEMS, max_iter, fixed_iters=0, poll_every=poll_every, **ir.LOOP_TEMS, **kw)


def same(got, want, tag):
    for what, a, b in zip(("out_sym", "converged", "iters", "passes_used"), got, want):
        assert np.array_equal(a, b), (tag, what, np.flatnonzero(np.asarray(a).reshape(len(a), -1) != np.asarray(b).reshape(len(b), -1))[:8])


@pytest.mark.parametrize("poll_every", [0, 2])
@pytest.mark.parametrize("cell", sorted(ir.LOOP_CELLS) + sorted(ir.TEMS_CELLS))
def test_loop_equals_the_oracle_loop(oracle, cell, poll_every):
    sh, rx, sigma, _, ref = ir.loop_cell(cell)
    if cell in ir.LOOP_CELLS:
        assert ir.has_loop_mix(ref[1], ref[3]), cell
    dec = loop_decoder(cell, poll_every)
    got = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, "maxlog")
    print(f"{cell}: passes used {np.bincount(got[3], minlength=4)[1:].tolist()}, converged {int(got[1].sum())} of {len(got[1])}")
    same(got, ref, (cell, poll_every))
    two = dec.decode_samples_idd(rx, sigma, 2, "maxlog")                      # fewer passes: the frames pass 3 would have taken stop at 2
    late = ref[3] == 3
    for a, b in zip(two[:3], ref[:3]):
        assert np.array_equal(a[~late], b[~late])
    assert (two[3][late] == 2).all() and not two[1][late].any()
    dec.close()


@pytest.mark.parametrize("cell", sorted(ir.LOOP_CELLS))
def test_every_codeword_alone_equals_its_row(oracle, cell):
    sh, rx, sigma, _, ref = ir.loop_cell(cell)
    dec = loop_decoder(cell, 0)
    for b in range(rx.shape[0]):
        one = dec.decode_samples_idd(rx[b:b + 1], sigma, ir.LOOP_PASSES, "maxlog")
        same(one, [x[b:b + 1] for x in ref], (cell, b))
    dec.close()


@pytest.mark.parametrize("cell", sorted(ir.LOOP_CELLS))
def test_batch_of_1100_equals_the_small_batch_row_for_row(oracle, cell):
    """the decoder's own active list (from 1024 codewords, poll_every = 2) inside every pass, and the gather at a ragged count"""
    sh, rx, sigma, _, ref = ir.loop_cell(cell)
    reps = 1100 // rx.shape[0] + 1
    big = np.concatenate([rx] * reps)[:1100]
    dec = loop_decoder(cell, 2)
    got = dec.decode_samples_idd(big, sigma, ir.LOOP_PASSES, "maxlog")
    same(got, [np.concatenate([x] * reps)[:1100] for x in ref], cell)
    dec.close()


@pytest.mark.parametrize("cell", sorted(ir.LOOP_CELLS))
def test_resident_entry_point_equals_the_host_buffer_one(oracle, cell):
    """the samples a slot holds (the device channel's, 96 frames at the cell's sigma), through both entry points, on the settings of
    every loop cell; the GPU's own results hold the convergence mix; the slot's samples are not overwritten; with a transmitter the
    final words are where nbl_count_errors reads them and out_sym may be NULL"""
    sh, _, sigma, _, _ = ir.loop_cell(cell)
    B = 96
    dec = loop_decoder(cell, 2)
    rng = np.random.default_rng(9)
    state = rng.integers(1, 30000, (B, 3)).astype(np.uint32)
    dec._tx_L = sh["L"]
    dec.channel_batch(0, np.zeros((B, sh["L"]), dtype=np.uint8), state, sigma)
    rx = dec.read_slot_rx(0, 0, B)
    host = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, "maxlog")
    res = dec.decode_resident(0, sigma, B, passes=ir.LOOP_PASSES, soft="maxlog")
    same(res, host, "resident")
    print(f"{cell}: passes used {np.bincount(host[3], minlength=4)[1:].tolist()}, converged {int(host[1].sum())} of {B}")
    assert ir.has_loop_mix(host[1], host[3]), (cell, host[1].tolist(), host[3].tolist())
    assert sr.bits_equal(dec.read_slot_rx(0, 0, B), rx)
    plain = dec.decode_resident(0, sigma, B)
    for a, b in zip(plain, dec.decode_samples(rx, sigma)):
        assert np.array_equal(a, b)
    # with a transmitter (the all-zero word): the slot keeps the loop's final words
    code = dg.graph(ir.LOOP_CELLS[cell][0])[0]
    K = code.N - code.M
    dec.set_transmitter(gen=None, crc_len=0, random_msg=0, parallel=1, punct=[], mod_order=sh["M"], n_mod_sym=sh["L"])
    dec.transmit_batch(0, np.ones(B, dtype=np.uint16), state, sigma)
    rx2 = dec.read_slot_rx(0, 0, B)
    none, conv, its, used = dec.decode_resident(0, sigma, B, want_out=False, passes=ir.LOOP_PASSES)
    host2 = dec.decode_samples_idd(rx2, sigma, ir.LOOP_PASSES)
    assert none is None
    same((host2[0], conv, its, used), host2, "resident, out_sym NULL")
    es, eb, _ = dec.count_errors(0, B)
    assert np.array_equal(es, (host2[0][:, :K] != 0).sum(axis=1))
    assert np.array_equal(eb, np.array([sum(bin(int(v)).count("1") for v in row[:K]) for row in host2[0]]))
    dec.close()


@pytest.mark.parametrize("soft", ["maxlog", "logsum"])
def test_loop_under_logsum_runs(oracle, soft):
    """log-sum demodulator (and either soft metric): not pinned end to end; the outputs are well formed and pass 1 is the plain call"""
    cell = "il64_it3"
    sh, rx, sigma, _, _ = ir.loop_cell(cell)
    dec = loop_decoder(cell, 2, metric=ir.LOGSUM)
    plain = dec.decode_samples(rx, sigma)
    out, conv, its, used = dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES, soft)
    assert ((used >= 1) & (used <= ir.LOOP_PASSES)).all() and (used[conv == 0] == ir.LOOP_PASSES).all()
    first = used == 1
    assert first.any() and np.array_equal(conv[first], plain[1][first]) and conv[first].all()
    assert np.array_equal(out[first], plain[0][first]) and np.array_equal(its[first], plain[2][first])
    assert (plain[1][~first] == 0).all() and ((out >= 0) & (out < sh["q"])).all() and ((its >= 1) & (its <= 3)).all()
    dec.close()


@pytest.mark.parametrize("soft", ["maxlog", "logsum"])
def test_one_pass_from_the_decoders_own_extrinsic(oracle, soft):
    """one step of the loop by hand under the log-sum demodulator: the extrinsic bit LLRs of a decode as the next prior; the L_ch of
    the second pass against the restatement from the SAME prior, within the log-sum tolerance"""
    cell = "il64_it3"
    sh, rx, sigma, _, _ = ir.loop_cell(cell)
    dec = loop_decoder(cell, 0, metric=ir.LOGSUM)
    dec.decode_samples(rx, sigma)
    sym, prior = dec.soft_output(soft, extrinsic=True)
    want_prior = sr.bit_marginals(sym, sh["p"], METRICS[soft], np.longdouble)
    assert sr.logsum_error(prior, want_prior, sym) <= sr.LOGSUM_TOL and np.abs(prior).max() > 1.0
    dec.decode_samples(rx, sigma, prior=prior)
    got = lch(dec, rx.shape[0])
    want, scale = ir.demod_prior(sh["points"], sh["src"], rx, sigma, sh["N"], sh["p"], ir.LOGSUM, prior, np.longdouble)
    err = np.abs(got - want)
    print(f"second pass, {soft} prior: worst error / scale = {float((err / np.where(scale > 0, scale, 1.0)).max()) / 2.0 ** -53:.2f} units of 2^-53")
    assert (err <= ir.LOGSUM_TOL * scale).all()
    dec.close()


# ---- state hygiene and refusals -------------------------------------------------------------------------------------------------
def test_state_after_a_loop_call(oracle):
    cell = "il64_it3"
    sh, rx, sigma, _, ref = ir.loop_cell(cell)
    dec = loop_decoder(cell, 2)
    before = dec.decode_samples(rx, sigma)
    soft_before = dec.soft_output("maxlog")
    state_before = dec.read_state(3, post=False, v2c=False)[2]
    ws = dec.workspace_bytes()
    dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES)
    assert dec.workspace_bytes() > ws                                         # the loop's buffers count from the moment they exist
    for call in (lambda: dec.soft_output("maxlog"), lambda: dec.soft_output("maxlog", extrinsic=True), lambda: dec.read_state(0, post=False, v2c=False)):
        with pytest.raises(nb.NblError) as e:
            call()
        assert e.value.status == -1 and "iterative-demapping loop" in str(e.value) and "ordinary decode call" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output_device("maxlog", None, 8)
    assert e.value.status == -1 and "iterative-demapping loop" in str(e.value)
    after = dec.decode_samples(rx, sigma)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for a, b in zip(soft_before, dec.soft_output("maxlog")):
        assert sr.bits_equal(a, b)
    assert sr.bits_equal(state_before, dec.read_state(3, post=False, v2c=False)[2])
    ws = dec.workspace_bytes()
    dec.decode_samples_idd(rx, sigma, ir.LOOP_PASSES)
    assert dec.workspace_bytes() == ws                                        # nothing grows the second time
    dec.close()


def test_refusals(oracle):
    cell = "il64_it3"
    sh, rx, sigma, _, _ = ir.loop_cell(cell)
    name = ir.LOOP_CELLS[cell][0]
    code = dg.graph(name)[0]
    B = 4
    rx = np.ascontiguousarray(rx[:B])
    out = np.zeros((B, code.N), dtype=np.int32)
    dec = nb.Decoder(code, nb.METHOD_EMS, 3, **ir.LOOP_EMS)
    lib = dec.lib

    def idd_call(passes, soft, idd_null=False):
        idd = nb.binding.IddParams(passes, soft)
        return lib.nbl_decode_batch_samples_idd(dec.h, rx.ctypes.data, sigma, B, None if idd_null else idd, out.ctypes.data, None, None, None)

    def res_call(passes, soft, idd_null=False):
        idd = nb.binding.IddParams(passes, soft)
        return lib.nbl_decode_batch_resident_idd(dec.h, 0, sigma, B, None if idd_null else idd, out.ctypes.data, None, None, None)

    def text():
        return lib.nbl_last_error(dec.h).decode()
    for call, who in ((idd_call, "nbl_decode_batch_samples_idd"), (res_call, "nbl_decode_batch_resident_idd")):
        assert call(3, 1) == -1 and who in text() and "nbl_set_demodulator has not been called" in text()      # no demodulator
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
    for call, who in ((idd_call, "nbl_decode_batch_samples_idd"), (res_call, "nbl_decode_batch_resident_idd")):
        assert call(3, 1, idd_null=True) == -1 and who in text() and "idd is NULL" in text()
        assert call(0, 1) == -1 and who in text() and "passes must be at least 1, got 0" in text()
        assert call(-2, 1) == -1 and "got -2" in text()
        assert call(3, 2) == -1 and who in text() and "unknown soft_metric 2" in text()
    assert lib.nbl_decode_batch_samples_idd(None, rx.ctypes.data, sigma, B, None, out.ctypes.data, None, None, None) == -1
    assert res_call(3, 1) == -1 and "slot does not hold" in text()             # what the plain resident call refuses, the same way
    assert idd_call(3, 1) == 0                                                # and the handle is usable
    # an unknown flag bit of the extrinsic call
    dec.decode_samples(rx, sigma)
    for flags in (2, 3, 0x80000000):
        with pytest.raises(nb.NblError) as e:
            dec.soft_output("maxlog", extrinsic=flags)
        assert e.value.status == -1 and "unknown flag bits" in str(e.value) and hex(flags & ~1) in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output_device("maxlog", 8, 8, extrinsic=4)
    assert e.value.status == -1 and "unknown flag bits 0x4" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output(2, extrinsic=True)
    assert e.value.status == -1 and "unknown metric 2" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output("maxlog", sym=False, bits=False, extrinsic=True)
    assert e.value.status == -1 and "both NULL" in str(e.value)
    dec.close()
    # method 6 has no messages: passes > 1 is unsupported, passes = 1 is the plain call; its extrinsic output is refused like the other
    sh, rx, _ = ir.kernel_case("gf16_qpsk_aligned")
    osd = nb.Decoder(nb.Code(dg.U16), nb.METHOD_OSD, 3, osd_order=1)
    osd.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
    with pytest.raises(nb.NblError) as e:
        osd.decode_samples_idd(rx, sigma, 2)
    assert e.value.status == -2 and "method 6" in str(e.value) and "passes must be 1" in str(e.value)
    one = osd.decode_samples_idd(rx, sigma, 1)
    for a, b in zip(one, osd.decode_samples(rx, sigma)):
        assert np.array_equal(a, b)
    with pytest.raises(nb.NblError) as e:
        osd.soft_output("maxlog", extrinsic=True)
    assert e.value.status == -2 and "method 6" in str(e.value)
    osd.close()


# ---- the harness switches ---------------------------------------------------------------------------------------------------------
HARNESS_KW = dict(gfq=256, method=2, max_iter=4, parallel=8, nqam=64, crc_len=8, random_msg=1, ems_nm=32, ems_nc=2, min_sim_cycle=320,
                  snr_begin=8.0, snr_step=1.0, snr_stop=8.0)   # 8 dB: about half of the frames converge in 4 iterations (the oracle)


@pytest.mark.parametrize("device_noise", ["1", "0"])
def test_harness_routes_both_decode_calls_through_the_loop(tmp_path, monkeypatch, device_noise):
    """NBL_IDD_PASSES=2 on GF(256) over Gray 64-QAM (a symbol straddles points): the harness's counts are those of the same frames (the
    host link chain's, lane after lane) through decode_samples_idd(passes=2), counted by the host chain's ErrCount -- with the channel
    on the device (DecodingBatchResident) and with host samples (DecodingBatchSamples); and they are not the counts of passes = 1"""
    from nbldpc_amd import hostlib
    monkeypatch.setenv("NBL_DEMOD_METRIC", "maxlog")
    monkeypatch.setenv("NBL_DEVICE_NOISE", device_noise)
    hostlib.prepare_workdir(str(tmp_path), HARNESS_KW, dg.U256, "GRAY_64QAM")
    code = nb.Code(dg.U256)
    N, K, P, p, m = code.N, code.N - code.M, 8, 8, 6
    L = N * p // m
    points = dg.named_points("GRAY_64QAM")
    src = dg.src_table(N, p, (), m, L)
    rows = {}
    for passes in ("1", "2"):
        monkeypatch.setenv("NBL_IDD_PASSES", passes)
        rows[passes] = hostlib.simulate(str(tmp_path))
        assert len(rows[passes]) == 1
    monkeypatch.delenv("NBL_IDD_PASSES")
    assert rows["1"] == hostlib.simulate(str(tmp_path))                       # the default is 1
    r = rows["2"][0]
    frames = int(r["frames"])
    assert frames >= 320 and frames % P == 0 and 0 < r["errFrame"] < frames, r
    _, _, msg, sigma = hostlib.frontend(str(tmp_path), 8.0, frames // P, N, K, code.q, P)
    rx, _, _, sigma2 = hostlib.channel(str(tmp_path), 8.0, frames // P, L, P)
    assert sigma == sigma2
    dec = nb.Decoder(code, nb.METHOD_EMS, 4, poll_every=2, ems_nm=32, ems_nc=2)
    dec.set_demodulator(64, L, src, points, metric=dg.MAXLOG)
    for passes in (1, 2):
        out, conv, its, used = dec.decode_samples_idd(rx, sigma, passes)
        es, eb, _ = hostlib.err_count(str(tmp_path), msg, out)
        h = rows[str(passes)][0]
        print(f"passes {passes}: harness", h, "own", int((es != 0).sum()), int(es.sum()), int(eb.sum()), "passes used", np.bincount(used).tolist())
        assert int(h["frames"]) == frames
        assert (h["errFrame"], h["errSym"], h["errBit"]) == (int((es != 0).sum()), int(es.sum()), int(eb.sum())), (passes, h)
    dec.close()
    assert (rows["1"][0]["errSym"], rows["1"][0]["errBit"]) != (r["errSym"], r["errBit"])   # the second pass changed decoded words


def test_harness_switch_refusals(tmp_path, monkeypatch, capfd):
    """every value the harness refuses, with its text: a pass count that is no integer from 1 up, an unknown soft metric, more than one
    pass without a general demodulator (BPSK), more than one pass with the demodulator on the host"""
    from nbldpc_amd import hostlib

    def refused(text):
        capfd.readouterr()
        with pytest.raises(RuntimeError):
            hostlib.simulate(str(tmp_path))
        err = capfd.readouterr().err
        assert text in err, (text, err)
    monkeypatch.setenv("NBL_DEMOD_METRIC", "maxlog")
    hostlib.prepare_workdir(str(tmp_path), HARNESS_KW, dg.U256, "GRAY_64QAM")
    for bad in ("0", "-1", "two", "2x", ""):
        monkeypatch.setenv("NBL_IDD_PASSES", bad)
        refused(f"NBL_IDD_PASSES={bad}: the number of demapping passes must be an integer from 1 up")
    monkeypatch.setenv("NBL_IDD_PASSES", "2")
    monkeypatch.setenv("NBL_IDD_SOFT", "exact")
    refused("NBL_IDD_SOFT=exact: unknown metric (maxlog, logsum)")
    monkeypatch.setenv("NBL_IDD_SOFT", "logsum")
    monkeypatch.setenv("NBL_DEVICE_DEMOD", "0")
    refused("NBL_IDD_PASSES=2: iterative demapping runs behind the device-side demodulator")
    monkeypatch.delenv("NBL_DEVICE_DEMOD")
    assert len(hostlib.simulate(str(tmp_path))) == 1                          # logsum, two passes: runs
    bpsk = tmp_path / "bpsk"
    bpsk.mkdir()
    hostlib.prepare_workdir(str(bpsk), dict(gfq=16, method=2, max_iter=4, ems_nm=8, ems_nc=2, parallel=8, crc_len=8, random_msg=1, min_sim_cycle=16,
                                            snr_begin=3.0, snr_step=1.0, snr_stop=3.0), dg.U16, "BPSK")
    capfd.readouterr()
    with pytest.raises(RuntimeError):
        hostlib.simulate(str(bpsk))
    assert "NBL_IDD_PASSES=2: iterative demapping needs the general demodulator" in capfd.readouterr().err
    monkeypatch.setenv("NBL_IDD_PASSES", "1")
    assert len(hostlib.simulate(str(bpsk))) == 1
