"""Bit-LLR input and batched soft output on a real MI355X (nbl_decode_batch_bits, nbl_soft_output; nbl_soft.hip) against the numpy
restatement of include/nbldpc.h's definition (tests/soft_ref.py) and, where a bit-exact CPU reference of the messages exists (EMS and
T-EMS, flooding and layered), against the sum over the ORACLE's c2v.  The grid and its frames are tests/soft_cases.py's: the shapes are
the smallest at which each kernel family and each c2v buffer rule can still go wrong (fused GF(256) kernels with double-buffered c2v,
small-field fused kernels, four checks per wave, the general kernels with the separate variable-node pass on degrees 1-8, layered,
OSD, the active list from B = 1024, max_iter = 0), each under early exit without and with polling and under fixed iterations.

Log-sum figures of the MI355X (worst |GPU - longdouble restatement| / max(1, max |P[n]|) over the whole grid): see
soft_ref.GPU_LOGSUM_ERR; every case prints its own before it asserts."""
import numpy as np
import pytest

import nbldpc_amd as nb
import layered_ref as lr
import soft_ref as sr
import soft_cases as sc
from test_gpu_parity import _force_generic

pytestmark = pytest.mark.gpu


def _decide_all(sym_b):
    return np.array([lr._decide(v) for v in sym_b], dtype=np.int32)


def check_soft(dec, name, method, mode, L, got, tag, sample=None, record=False):
    """assertions 1-5 of a decode that has just run on `dec`; returns the worst log-sum error"""
    out, conv, its = got
    code, edges, _ = sc.graph(name)
    p = code.q.bit_length() - 1
    B = L.shape[0]
    fixed = sc.MODES[mode].get("fixed_iters", 0)
    sym, bits = dec.soft_output("maxlog")
    sym2, bits_ls = dec.soft_output("logsum")
    assert sym.shape == (B, code.N, code.q - 1) and bits.shape == (B, code.N * p)
    assert sr.bits_equal(sym, sym2), tag
    import pyoracle
    g = lr.Graph(pyoracle.Code(edges=edges))
    # 1. the definition on the decoder's own state, bit for bit (and 3: record_state's post on converged frames)
    for b in (range(B) if sample is None else sample):
        post, _, c2v = dec.read_state(b, post=record, v2c=False)
        assert sr.bits_equal(sym[b], sr.posterior(dec.read_lch(b), c2v, g)), (tag, b, "definition")
        if conv[b] and not fixed:
            assert np.array_equal(_decide_all(sym[b]), out[b]), (tag, b, "decision")
            if record:
                assert sr.bits_equal(sym[b], post), (tag, b, "post")
    # 2. the same sum over the oracle's c2v
    if method in sc.EXACT:
        ref = sc.oracle_state(name, "ems" if method == "ems1100" else method, fixed)
        for b in (range(B) if sample is None else sample):
            r_conv, r_its, r_out, r_c2v = ref[b % len(sc.frames(name)[0])] if method == "ems1100" else ref.get(b, (None,) * 4)
            if r_conv is None:
                continue                                            # (a frame outside the oracle's sample)
            assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
            if method != "osd" or r_conv:
                assert np.array_equal(out[b], r_out), (tag, b)      # 4: OSD changes out_sym of the unconverged frames only
            assert sr.bits_equal(sym[b], sr.posterior(L[b], r_c2v, g)), (tag, b, "oracle")
    # 5. bit marginals
    assert sr.bits_equal(bits, sr.bit_marginals(sym, p, sr.MAXLOG)), (tag, "max-log")
    err = sr.logsum_error(bits_ls, sr.bit_marginals(sym, p, sr.LOGSUM, np.longdouble), sym)
    print(f"{tag}: log-sum error {err:.3e} = {err * 2.0 ** 53:.2f} units of 2^-53 (tolerance {sr.LOGSUM_TOL:.3e})")
    assert err <= sr.LOGSUM_TOL, (tag, err)
    return err


def assert_mix(name, method, conv, its, tag):
    o_conv, o_its = sc.oracle_flags(name, method)
    assert sc.has_mix(o_conv, o_its), (tag, "oracle", list(zip(o_conv.tolist(), o_its.tolist())))
    assert sc.has_mix(conv, its), (tag, "gpu", list(zip(conv.tolist(), its.tolist())))


@pytest.mark.parametrize("mode", sorted(sc.MODES))
@pytest.mark.parametrize("name,method,generic", sc.GRID)
def test_decoder_grid(oracle, name, method, generic, mode):
    L = sc.frames(name)[0]
    tag = (name, method, generic, mode)
    dec = sc.decoder(name, method, mode)
    _force_generic(dec, generic)
    record = mode == "poll2"
    dec.record_state(record)
    got = dec.decode(L)
    if not sc.MODES[mode].get("fixed_iters", 0):
        assert_mix(name, method, got[1], got[2], tag)
    check_soft(dec, name, method, mode, L, got, tag, record=record)
    dec.close()


def test_active_list_from_1024_frames(oracle):
    """EMS on the GF(16) code, B = 1100, poll_every = 2: the grids of the later windows cover the active list only; the soft pass
    covers every codeword"""
    L24 = sc.frames(sc.U16)[0]
    L = np.concatenate([L24] * 46)[:1100]
    dec = sc.decoder(sc.U16, "ems", "poll2")
    got = dec.decode(L)
    assert_mix(sc.U16, "ems", got[1][:24], got[2][:24], "ems1100")
    sample = list(range(48)) + list(range(1100 - 24, 1100))
    check_soft(dec, sc.U16, "ems1100", "poll2", L, got, "ems1100", sample=sample)
    sym, bits = dec.soft_output("maxlog")
    for b in range(1100):
        assert sr.bits_equal(sym[b], sym[b % 24]) and sr.bits_equal(bits[b], bits[b % 24]), b
    dec.close()


@pytest.mark.parametrize("mode", sorted(sc.MODES))
@pytest.mark.parametrize("name", [sc.U16, sc.U256])
def test_max_iter_zero(oracle, name, mode):
    """no iteration: P = L_ch (plus the zeros of iteration 0)"""
    L = sc.frames(name)[0]
    dec = sc.decoder(name, "ems", mode, max_iter=0)
    got = dec.decode(L)
    assert not got[1].any()
    check_soft(dec, name, None, mode, L, got, (name, "max_iter 0", mode))
    sym, _ = dec.soft_output("maxlog", bits=False)
    assert sr.bits_equal(sym, L + 0.0)
    dec.close()


@pytest.mark.parametrize("name,method,mode", [(sc.U256, "ems", "poll0"), (sc.U16, "tems", "poll2"), (sc.BDS, "bp", "fixed"),
                                              ("all8", "ems", "poll0")])
def test_host_and_device_entry_points_give_identical_bytes(oracle, name, method, mode):
    """the device form on a caller's stream with torch buffers, behind nbl_decode_batch_device on the same stream; NULL for either
    output is honoured and the other buffer is untouched (a canary)"""
    import torch
    L = sc.frames(name)[0]
    code = sc.graph(name)[0]
    B, p = L.shape[0], code.q.bit_length() - 1
    dec = sc.decoder(name, method, mode)
    host = dec.decode(L)
    h_sym, h_bits = dec.soft_output("maxlog")
    _, h_ls = dec.soft_output("logsum", sym=False)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dL = torch.from_numpy(np.array(L)).cuda()
        out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
        conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
        its = torch.zeros(B, dtype=torch.int32, device="cuda")
        canary = 12345.678
        sym = torch.full((B, code.N, code.q - 1), canary, dtype=torch.float64, device="cuda")
        bits = torch.full((B, code.N * p), canary, dtype=torch.float64, device="cuda")
        ls = torch.full((B, code.N * p), canary, dtype=torch.float64, device="cuda")
        sym_c, bits_c = sym.clone(), bits.clone()
        stream.synchronize()
        dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), stream.cuda_stream)
        dec.soft_output_device("maxlog", sym.data_ptr(), bits.data_ptr(), stream.cuda_stream)
        dec.soft_output_device("logsum", None, ls.data_ptr(), stream.cuda_stream)
        dec.soft_output_device(nb.SOFT_MAXLOG, sym_c.data_ptr(), None, stream.cuda_stream)
        stream.synchronize()
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    assert sr.bits_equal(sym.cpu().numpy(), h_sym) and sr.bits_equal(bits.cpu().numpy(), h_bits) and sr.bits_equal(ls.cpu().numpy(), h_ls)
    assert sr.bits_equal(sym_c.cpu().numpy(), h_sym) and bool((bits_c == canary).all())
    # host form: None for either output
    s_only, none = dec.soft_output("maxlog", bits=False, B=B)
    assert none is None and sr.bits_equal(s_only, h_sym)
    none, b_only = dec.soft_output("maxlog", sym=False, B=B)
    assert none is None and sr.bits_equal(b_only, h_bits)
    dec.close()


@pytest.mark.parametrize("name", ["all4", sc.U16, sc.BDS, sc.U256])
def test_bits_input(oracle, name):
    """q = 4, 16, 64, 256: the L_ch the decoder holds after decode_bits(lam) is the restatement's expansion bit for bit (it is also the
    host chain's own L_ch of these frames), and the decode equals that of the expanded input; host and device form agree"""
    import torch
    L, lam = sc.frames(name)
    code = sc.graph(name)[0]
    p = code.q.bit_length() - 1
    B = L.shape[0]
    want = sr.bits_to_lch(lam, p)
    assert sr.bits_equal(want, L)
    dec = sc.decoder(name, "ems", "poll2")
    ref = dec.decode(L)
    got = dec.decode_bits(lam)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    for b in range(B):
        assert sr.bits_equal(dec.read_lch(b), want[b]), (name, b)
    ws = dec.workspace_bytes()
    dl = torch.from_numpy(np.array(lam)).cuda()
    out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_bits_device(dl.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, b in zip(ref, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    assert dec.workspace_bytes() == ws                       # (the device form stages nothing)
    sym, bits = dec.soft_output("maxlog")
    assert dec.workspace_bytes() == ws + sym.nbytes + bits.nbytes   # the staging buffers count from the moment they exist
    dec.close()


def test_bits_input_equals_the_bpsk_demodulator(tmp_path, oracle):
    """lam formed from BPSK samples (Comm.cpp:356), one frame punctured by hand: decode_bits equals decode_samples, bit-identical L_ch"""
    from nbldpc_amd import hostlib
    code = sc.graph(sc.U16)[0]
    N, K, q, P = code.N, code.N - code.M, code.q, 6
    p = q.bit_length() - 1
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=q, code=sc.U16, method=2, max_iter=8, parallel=P, constellation="BPSK", random_msg=1), sc.U16, "BPSK")
    rx, _, _, sigma = hostlib.channel(str(tmp_path), 3.0, 1, N * p, P)
    src = np.arange(N * p, dtype=np.int32)
    src[5 * p:6 * p] = -1                                    # symbol 5 punctured: its bits are the caller's 0.0
    lam = -2 * rx[:, :, 0] / (sigma * sigma)
    lam[:, 5 * p:6 * p] = 0.0
    dec = sc.decoder(sc.U16, "ems", "poll0")
    dec.set_demodulator(2, N * p, src)
    a = dec.decode_samples(rx, sigma)
    La = np.stack([dec.read_lch(b) for b in range(P)])
    b = dec.decode_bits(lam)
    Lb = np.stack([dec.read_lch(b) for b in range(P)])
    assert sr.bits_equal(La, Lb) and not Lb[:, 5].any()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    dec.close()


def test_method_6(oracle):
    """an OSD-only decoder reads L_ch only: decode_bits equals decode of the expanded input; it has no soft output"""
    L, lam = sc.frames(sc.U16)
    code = sc.graph(sc.U16)[0]
    dec = nb.Decoder(code, nb.METHOD_OSD, 10, osd_order=1)
    ref = dec.decode(L)
    got = dec.decode_bits(lam)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output("maxlog")
    assert e.value.status == -2 and "method 6" in str(e.value)
    dec.close()


def test_refusals(oracle):
    L, lam = sc.frames(sc.U16)
    code = sc.graph(sc.U16)[0]
    dec = sc.decoder(sc.U16, "ems", "poll0")
    with pytest.raises(nb.NblError) as e:
        dec.soft_output("maxlog")
    assert e.value.status == -1 and "no decode call" in str(e.value)
    out = np.zeros((4, code.N), dtype=np.int32)
    lib = dec.lib
    assert lib.nbl_decode_batch_bits(dec.h, None, 4, out.ctypes.data, None, None) == -1
    assert lib.nbl_decode_batch_bits(dec.h, lam.ctypes.data, -1, out.ctypes.data, None, None) == -1
    assert lib.nbl_decode_batch_bits(dec.h, lam.ctypes.data, 4, None, None, None) == -1
    assert lib.nbl_decode_batch_bits(None, lam.ctypes.data, 4, out.ctypes.data, None, None) == -1
    assert lib.nbl_decode_batch_bits(dec.h, lam.ctypes.data, 0, out.ctypes.data, None, None) == 0
    assert lib.nbl_decode_batch_bits_device(dec.h, None, 4, out.ctypes.data, None, None, None) == -1
    assert lib.nbl_decode_batch_bits_device(dec.h, lam.ctypes.data, -1, out.ctypes.data, None, None, None) == -1
    with pytest.raises(nb.NblError) as e:                    # (B = 0 was no decode)
        dec.soft_output("maxlog")
    assert e.value.status == -1 and "no decode call" in str(e.value)
    dec.decode_bits(lam[:4])
    with pytest.raises(nb.NblError) as e:
        dec.soft_output("maxlog", sym=False, bits=False)
    assert e.value.status == -1 and "both NULL" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output(2)
    assert e.value.status == -1 and "unknown metric 2" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output_device(2, None, None)
    assert e.value.status == -1
    assert lib.nbl_soft_output(None, 1, out.ctypes.data, None) == -1
    sym, bits = dec.soft_output("maxlog")                    # and the handle is still usable
    assert sym.shape == (4, code.N, code.q - 1) and np.isfinite(sym).all() and np.isfinite(bits).all()
    dec.close()


@pytest.mark.parametrize("name,method", [(sc.U256, "ems"), (sc.U16, "bp")])
def test_soft_output_leaves_the_decoder_as_it_was(oracle, name, method):
    """a flooding decode's out / converged / iters / read_state are the same whether or not soft_output was called in between"""
    L = sc.frames(name)[0]
    dec = sc.decoder(name, method, "poll0")
    dec.record_state(True)
    first = dec.decode(L)
    state = [dec.read_state(b) for b in range(L.shape[0])]
    dec.soft_output("logsum")
    dec.soft_output("maxlog")
    for b in range(L.shape[0]):
        for x, y in zip(dec.read_state(b), state[b]):
            assert sr.bits_equal(x, y), (name, b)
    again = dec.decode(L)
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    for b in range(L.shape[0]):
        for x, y in zip(dec.read_state(b), state[b]):
            assert sr.bits_equal(x, y), (name, b)
    dec.close()
