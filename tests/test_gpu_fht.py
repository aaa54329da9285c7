"""FHT sum-product decoding on a real MI355X (nbl_create_fht; nbl_cn_fht.hip, nbl_cn_fht_layered.hip) against its numpy restatement
(tests/fht_ref.py), flooding and layered.  The parity statement is the method's own (include/nbldpc.h): out_sym, converged and iters
equal; post, c2v and v2c compared as w(x) = exp(x - max x), the probability-domain view, within 16 x the case's recorded deviation
between the restatement in FP64 and in 80-bit arithmetic (fht_ref.D80).  The GPU evaluates the same adds and products and differs only
in exp / log -- up to about 2 ulp, against the 0.5 ulp of libm that the recorded figure already contains: 4 x for that, 4 x for the
sample-to-sample spread of how a rounding is amplified.  Decision equality is meaningful on these inputs: tests/test_fht.py asserts that
no decision of any case used here is closer than 1e-6 to going the other way.  Shapes are those of tests/test_gpu_layered_bp.py, the
smallest that reach each code path."""
import os
import re
import subprocess

import numpy as np
import pytest

import nbldpc_amd as nb
import fht_ref as fr
import soft_ref
from test_fht import fht_case, fht_reference, tolerance
from test_gpu_layered import assignments

pytestmark = pytest.mark.gpu

SCHEDULES = ("flooding", "greedy")


def close_to(dec, got, ref, tol, tag, B=None):
    """every output of frames 0 .. B-1 of the last decode equal to the restatement's, the message state within `tol` in the probability
    domain; returns the largest deviation seen"""
    out, conv, its = got
    worst = 0.0
    for b in range(len(ref) if B is None else B):
        r_out, r_conv, r_its = ref[b][:3]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, v2c, c2v = dec.read_state(b)
        devs = {}
        for what, a, x in (("post", post, ref[b][3]), ("c2v", c2v, ref[b][4]), ("v2c", v2c, ref[b][5])):
            assert np.all(np.isfinite(a)), (tag, b, what)
            devs[what] = fr.w_dev(a, x)
        print(tag, "frame", b, "deviation in the probability domain:", devs, "tolerance", tol)
        worst = max(worst, max(devs.values()))
    print(tag, "largest deviation in the probability domain:", worst, "tolerance", tol)
    assert worst <= tol, (tag, worst, tol)
    return worst


def fht_decoder(name, which="flooding", **extra):
    code, L, iters = fht_case(name)
    layers = None if which == "flooding" else "greedy" if which == "greedy" else assignments(code)[which]
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=layers, fht=True, **extra)
    dec.record_state(True)
    return dec, L


@pytest.mark.parametrize("which", SCHEDULES)
def test_gf16_frames_that_converge_at_different_iterations(oracle, which):
    """Shipped GF(16) code, 8 frames at 1.5 dB, 8 iterations: frames converge at different iterations and never; iters is checked per
    frame.  Launches per iteration: variable-node pass (or decision), syndrome, one check-node launch (or one per layer)."""
    ref = fht_reference("gf16", which)
    dec, L = fht_decoder("gf16", which)
    close_to(dec, dec.decode(L), ref, tolerance("gf16", which), ("gf16", which))
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 8 and n_cn == 8 * (1 if which == "flooding" else int(dec.layers.max()) + 1)
    assert (dec.layers is None) == (which == "flooding")
    dec.close()


@pytest.mark.parametrize("which", ["flooding", "greedy", "serial", "other"])
@pytest.mark.parametrize("name", ["ring256", "ring64"])
def test_ring_codes_normal_saturating_and_mixed(oracle, name, which):
    """_ring_code(256, 8, 4) (four symbols per lane) and _ring_code(64, 8, 4) (one): 3 frames -- normal(-2, 4), normal(-900, 700) (every
    vector one-hot, the outputs at the floor), narrow and wide vectors mixed in one check -- 3 iterations, flooding and under the three
    assignments."""
    dec, L = fht_decoder(name, which)
    close_to(dec, dec.decode(L), fht_reference(name, which), tolerance(name, which), (name, which))
    if which != "flooding":
        assert np.array_equal(dec.layers, assignments(fht_case(name)[0])[which])
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
@pytest.mark.parametrize("name", ["all-4", "all-8", "all-16", "dv48-32", "rand128"])
def test_degrees_and_fields(oracle, name, which):
    """The `all` degree profile (checks of degree 2-8, variables of degree 1-8) over GF(4), GF(8), GF(16); variables of degree 4-8 over
    GF(32); an irregular graph over GF(128) (two symbols per lane).  One real-valued frame, 3 iterations."""
    code = fht_case(name)[0]
    if name.startswith("all"):
        assert code.var_deg.min() == 1 and code.var_deg.max() == 8 and (code.chk_deg.min(), code.chk_deg.max()) == (2, 8)
    dec, L = fht_decoder(name, which)
    close_to(dec, dec.decode(L), fht_reference(name, which), tolerance(name, which), (name, which))
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_fixed_iterations(oracle, which):
    """fixed_iters = 1: every frame runs max_iter iterations, its outputs frozen at the first zero syndrome, its state that of
    iteration 8; against the restatement's fixed mode."""
    ref, early = fht_reference("gf16", which, 1), fht_reference("gf16", which)
    assert any(r[1] and r[2] < 8 for r in ref)
    for r, e in zip(ref, early):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[5], e[5])      # (a frame that converged early went on iterating)
    dec, L = fht_decoder("gf16", which, fixed_iters=1)
    close_to(dec, dec.decode(L), ref, tolerance("gf16", which, 1), ("fixed", which))
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_poll_every_and_batches_of_one_and_five(oracle, which):
    ref = fht_reference("gf16", which)
    tol = tolerance("gf16", which)
    for poll in (1, 3):
        dec, L = fht_decoder("gf16", which, poll_every=poll)
        close_to(dec, dec.decode(L), ref, tol, ("poll", poll, which))
        dec.close()
    dec, L = fht_decoder("gf16", which)
    for B in (1, 5):
        close_to(dec, dec.decode(L[:B]), ref, tol, ("B", B, which), B=B)
    dec.close()


@pytest.mark.parametrize("which", SCHEDULES)
def test_device_buffers_equal_host_buffers(oracle, which):
    import torch
    ref = fht_reference("gf16", which)
    dec, L = fht_decoder("gf16", which)
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
    """decode_bits equals decode on the expanded LLRs; the symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit the sum
    formed from this decoder's own c2v (nbl_read_state) in the header's order."""
    code = fht_case("gf16")[0]
    p = code.q.bit_length() - 1
    sigma = 0.95
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
    dec.close()


def test_fht_and_exact_decoders_agree_in_decisions_and_differ_in_messages(oracle):
    """An FHT decoder and an exact log-QSPA decoder on `gf16`: converged and out_sym agree on every frame both converge on, while their
    c2v differ -- the kernel really is another one.  nbl_get_layers is NBL_ERR_ARG on the flooding kind."""
    code, L, iters = fht_case("gf16")
    for which in SCHEDULES:
        dec, _ = fht_decoder("gf16", which)
        f_out, f_conv, _ = dec.decode(L)
        f_c2v = [dec.read_state(b)[2] for b in range(L.shape[0])]
        dec.close()
        exact = nb.Decoder(code, nb.METHOD_BP, iters, **({} if which == "flooding" else dict(layers="greedy", bp=True)))
        exact.record_state(True)
        e_out, e_conv, _ = exact.decode(L)
        both = [b for b in range(L.shape[0]) if f_conv[b] and e_conv[b]]
        assert len(both) >= 3, (which, f_conv, e_conv)
        for b in both:
            assert np.array_equal(f_out[b], e_out[b]), (which, b)
        differ = [b for b in range(L.shape[0]) if not np.array_equal(exact.read_state(b)[2], f_c2v[b])]
        assert len(differ) >= L.shape[0] - 1, (which, differ)    # (a frame that converges at iteration 1 has all-zero c2v in both)
        exact.close()
    flood = nb.Decoder(code, nb.METHOD_BP, iters, fht=True)
    assert flood.layers is None
    flood.close()


def _harness(workdir, env):
    """nbldpc_sim in `workdir` under the environment `env`: (return code, iterations per frame of its report | None, its output)"""
    from nbldpc_amd import hostlib
    r = subprocess.run([hostlib.SIM_BIN], cwd=workdir, env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    m = re.search(r"\(([0-9.eE+-]+) iterations per frame\)", r.stdout)
    return r.returncode, float(m.group(1)) if m else None, r.stdout + r.stderr


def test_harness_check_node_switch(tmp_path, monkeypatch):
    """NBL_BP_CHECK=fht in the host layer: the harness (nbldpc_sim) on the shipped GF(16) code, log-QSPA, 30 iterations, BPSK at 2 dB,
    8 lanes, flooding and under NBL_SCHEDULE=layered-bp.  Its counts (the same main loop through hostlib.simulate) are those of the
    same frames decoded by Decoder(fht=True) and counted by the host chain's ErrCount, its iterations per frame their mean.  An EMS
    profile under the switch, and an unknown value, are refused with a message."""
    from nbldpc_amd import hostlib
    from test_layered import GF16
    code = nb.Code(GF16)
    N, K, P = code.N, code.N - code.M, 8
    kw = dict(gfq=16, method=nb.METHOD_BP, max_iter=30, parallel=P, crc_len=8, random_msg=1, min_sim_cycle=320, snr_begin=2.0, snr_step=1.0,
              snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    for sched, layers in (("flooding", None), ("layered-bp", "greedy")):
        env = dict(NBL_BP_CHECK="fht", NBL_SCHEDULE=sched)
        rc, mean, text = _harness(str(tmp_path), env)
        assert rc == 0 and mean is not None and mean > 1.0, text
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rows = hostlib.simulate(str(tmp_path))
        assert len(rows) == 1
        r = rows[0]
        frames = int(r["frames"])
        assert frames >= 320 and frames % P == 0
        L, tx, msg, _ = hostlib.frontend(str(tmp_path), 2.0, frames // P, N, K, code.q, P)
        dec = nb.Decoder(code, nb.METHOD_BP, 30, poll_every=2, layers=layers, fht=True)
        out, conv, its = dec.decode(L)
        dec.close()
        err_sym, err_bit, _ = hostlib.err_count(str(tmp_path), msg, out)
        print("harness", sched, r, "own", int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum()), "iterations per frame", its.mean())
        assert (r["errFrame"], r["errSym"], r["errBit"]) == (int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum())), r
        assert abs(mean - its.mean()) <= 1e-4 * its.mean()
    rc, _, text = _harness(str(tmp_path), dict(NBL_BP_CHECK="fft"))
    assert rc != 0 and "unknown check node" in text, text
    rc, _, text = _harness(str(tmp_path), dict(NBL_BP_CHECK="fht", NBL_SCHEDULE="layered"))
    assert rc != 0 and "NBL_BP_CHECK=fht" in text, text
    ems = tmp_path / "ems"
    ems.mkdir()
    hostlib.prepare_workdir(str(ems), dict(kw, method=nb.METHOD_EMS), GF16, "BPSK")
    rc, _, text = _harness(str(ems), dict(NBL_BP_CHECK="fht"))
    assert rc != 0 and "log-QSPA (method 1)" in text, text
