"""The damped layered (check-serial) log-QSPA schedule on a real MI355X (nbl_create_layered_bp, nbl_cn_bp_layered.hip) against its numpy
restatement (tests/layered_bp_ref.py, which takes the per-check update from the oracle's FP64 log-QSPA check).  The parity statement is
the method's own (tests/test_gpu_parity.py): out_sym, converged and iters equal; post, c2v and v2c within LLR_TOL = 1e-9 of the largest
magnitude of the compared array.  Decision equality is meaningful on these inputs: tests/test_layered_bp.py asserts that no decision
of any case used here is closer than 1e-6 to going the other way.  Shapes are the smallest that reach each code path: the shipped
GF(16) code, ring graphs over GF(64) and GF(256) (one and four symbols per lane) with narrow, wide and mixed inputs, the `all` degree
profile (checks 2-8, variables 1-8) over GF(4), GF(8) and GF(16), variables of degree 4-8 over GF(32), two symbols per lane at
GF(128)."""
import os
import re
import subprocess

import numpy as np
import pytest

import nbldpc_amd as nb
import soft_ref
from test_gpu_layered import assignments
from test_gpu_parity import LLR_TOL
from test_layered_bp import case, flooding, reference

pytestmark = pytest.mark.gpu


def close_to(dec, got, ref, tag, B=None):
    """every output of frames 0 .. B-1 of the last decode equal to the restatement's, the message state within LLR_TOL; returns the
    largest deviation seen, relative to the largest magnitude of its array"""
    out, conv, its = got
    worst = 0.0
    for b in range(len(ref) if B is None else B):
        r_out, r_conv, r_its = ref[b][:3]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, v2c, c2v = dec.read_state(b)
        for what, a, x in (("post", post, ref[b][3]), ("c2v", c2v, ref[b][4]), ("v2c", v2c, ref[b][5])):
            assert np.all(np.isfinite(a)), (tag, b, what)
            dev = np.max(np.abs(a - x)) / max(1.0, np.max(np.abs(x)))
            worst = max(worst, dev)
            assert dev <= LLR_TOL, (tag, b, what, dev)
    print(tag, "largest deviation / largest magnitude:", worst)
    return worst


def layered(name, which="greedy", **extra):
    code, L, iters = case(name)
    dec = nb.Decoder(code, nb.METHOD_BP, iters, layers="greedy" if which == "greedy" else assignments(code)[which], bp=True, **extra)
    dec.record_state(True)
    return dec, L


def test_gf16_frames_that_converge_at_different_iterations(oracle):
    """Shipped GF(16) code, 8 frames at 1.5 dB, 8 iterations, greedy layers: frames 3, 4, 6 and 7 converge at iterations 7, 4, 2 and 4,
    the other four do not; iters is checked per frame, the state of a converged frame is what iteration iters - 1 left.  Launches per
    iteration: decision, syndrome, one per layer."""
    ref = reference("gf16", "greedy")
    assert [(r[1], r[2]) for r in ref] == [(0, 8), (0, 8), (0, 8), (1, 7), (1, 4), (0, 8), (1, 2), (1, 4)]
    dec, L = layered("gf16")
    close_to(dec, dec.decode(L), ref, "gf16")
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 8 and n_cn == 8 * (int(dec.layers.max()) + 1)
    dec.close()


@pytest.mark.parametrize("which", ["greedy", "serial", "other"])
@pytest.mark.parametrize("name", ["ring256", "ring64"])
def test_ring_codes_under_three_assignments(oracle, name, which):
    """_ring_code(256, 8, 4) (four symbols per lane) and _ring_code(64, 8, 4): 3 frames -- normal(-2, 4), normal(-900, 700) (the
    mantissa / exponent path of the convolutions), narrow and wide vectors mixed in one check -- 3 iterations, under the greedy
    assignment, one layer per check, and a caller's assignment that is neither."""
    dec, L = layered(name, which)
    close_to(dec, dec.decode(L), reference(name, which), (name, which))
    assert np.array_equal(dec.layers, assignments(case(name)[0])[which])
    dec.close()


@pytest.mark.parametrize("name", ["all-4", "all-8", "all-16", "dv48-32", "rand128"])
def test_degrees_and_fields(oracle, name):
    """The `all` degree profile (checks of degree 2-8, variables of degree 1-8) over GF(4), GF(8), GF(16); variables of degree 4-8
    (up to eight c2v vectors summed per input) over GF(32); an irregular graph over GF(128) (two symbols per lane).  One real-valued
    frame, 3 iterations."""
    code = case(name)[0]
    if name.startswith("all"):
        assert code.var_deg.min() == 1 and code.var_deg.max() == 8 and (code.chk_deg.min(), code.chk_deg.max()) == (2, 8)
    if name.startswith("dv48"):
        assert (code.var_deg.min(), code.var_deg.max()) == (4, 8)
    dec, L = layered(name)
    close_to(dec, dec.decode(L), reference(name, "greedy"), name)
    dec.close()


def test_fixed_iterations(oracle):
    """fixed_iters = 1: every frame runs max_iter iterations, its outputs frozen at the first zero syndrome, its state (c2v and v2c)
    that of iteration 8; against the restatement's fixed mode."""
    ref, early = reference("gf16", "greedy", 1), reference("gf16", "greedy")
    assert any(r[1] and r[2] < 8 for r in ref)
    for r, e in zip(ref, early):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 8 or not np.array_equal(r[5], e[5])      # (a frame that converged early went on iterating)
    dec, L = layered("gf16", fixed_iters=1)
    close_to(dec, dec.decode(L), ref, "fixed")
    dec.close()


def test_poll_every_does_not_change_results(oracle):
    ref = reference("gf16", "greedy")
    for poll in (1, 3):
        dec, L = layered("gf16", poll_every=poll)
        close_to(dec, dec.decode(L), ref, ("poll", poll))
        dec.close()


def test_batches_of_one_and_five(oracle):
    ref = reference("gf16", "greedy")
    dec, L = layered("gf16")
    for B in (1, 5):
        close_to(dec, dec.decode(L[:B]), ref, ("B", B), B=B)
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
    close_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, "device")
    state = [dec.read_state(b) for b in range(B)]
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    for b in range(B):                                  # the same kernels on the same numbers: bit for bit
        for a, x in zip(dec.read_state(b), state[b]):
            assert np.array_equal(a, x), b
    dec.close()


def test_bit_llr_input_and_soft_output(oracle):
    """decode_bits equals decode on the expanded LLRs; the symbol LLRs of nbl_soft_output, plain and extrinsic, are bit for bit the sum
    formed from this decoder's own c2v (nbl_read_state) in the header's order: L_ch (or 0.0), then the variable's edges in its order."""
    code = case("gf16")[0]
    p = code.q.bit_length() - 1
    sigma = 0.95                                        # (chosen on the CPU with the restatement: frame 0 converges at iteration 3, the others do not)
    lam = -2.0 * (1.0 + sigma * np.random.default_rng(78).standard_normal((4, code.N * p))) / sigma ** 2
    L = soft_ref.bits_to_lch(lam, p)
    dec = nb.Decoder(code, nb.METHOD_BP, 4, layers="greedy", bp=True)
    dec.record_state(True)
    want = dec.decode(L)
    state = [dec.read_state(b) for b in range(4)]
    got = dec.decode_bits(lam)
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert list(zip(want[1], want[2])) == [(1, 3), (0, 4), (0, 4), (0, 4)]

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


def test_get_layers_and_flooding_differs(oracle):
    """nbl_get_layers returns the assignment in use; a flooding decoder on the same inputs is another decoder (other iteration counts),
    still equal to the flooding oracle's."""
    code, L, iters = case("gf16")
    for which, lay in assignments(code).items():
        dec = nb.Decoder(code, nb.METHOD_BP, iters, layers=lay, bp=True)
        assert np.array_equal(dec.layers, lay), which
        dec.close()
    dec, _ = layered("gf16")
    assert np.array_equal(dec.layers, nb.layer_greedy(code))
    _, conv, its = dec.decode(L)
    dec.close()
    flood = nb.Decoder(code, nb.METHOD_BP, iters)
    assert flood.layers is None
    _, f_conv, f_its = flood.decode(L)
    flood.close()
    assert [(c, i) for c, i in zip(f_conv, f_its)] == [f[:2] for f in flooding("gf16")]
    assert not np.array_equal(f_its, its)


def _harness(workdir, sched):
    """nbldpc_sim in `workdir` under NBL_SCHEDULE=sched: (return code, iterations per frame of its report | None, its output)"""
    from nbldpc_amd import hostlib
    r = subprocess.run([hostlib.SIM_BIN], cwd=workdir, env=dict(os.environ, NBL_SCHEDULE=sched), capture_output=True, text=True, timeout=120)
    m = re.search(r"\(([0-9.eE+-]+) iterations per frame\)", r.stdout)
    return r.returncode, float(m.group(1)) if m else None, r.stdout + r.stderr


def test_harness_schedule_switch(tmp_path, monkeypatch):
    """NBL_SCHEDULE=layered-bp in the host layer: the harness (nbldpc_sim) on the shipped GF(16) code, log-QSPA, 30 iterations, BPSK at
    2 dB, 8 lanes, reports fewer iterations per frame than under NBL_SCHEDULE=flooding at the same seed.  Its counts (the same main
    loop through hostlib.simulate) are those of the same frames decoded by Decoder(layers="greedy", bp=True) and counted by the host
    chain's ErrCount, its iterations per frame their mean.  NBL_SCHEDULE=layered still refuses a log-QSPA profile."""
    from nbldpc_amd import hostlib
    from test_layered import GF16
    code = nb.Code(GF16)
    N, K, P = code.N, code.N - code.M, 8
    kw = dict(gfq=16, method=nb.METHOD_BP, max_iter=30, parallel=P, crc_len=8, random_msg=1, min_sim_cycle=320, snr_begin=2.0, snr_step=1.0,
              snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    rc_l, mean_l, text_l = _harness(str(tmp_path), "layered-bp")
    rc_f, mean_f, text_f = _harness(str(tmp_path), "flooding")
    print("harness iterations per frame: layered-bp", mean_l, "flooding", mean_f)
    assert rc_l == 0 and rc_f == 0 and mean_l is not None and mean_f is not None, (text_l, text_f)
    assert 1.0 < mean_l < mean_f
    monkeypatch.setenv("NBL_SCHEDULE", "layered-bp")
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == 1
    r = rows[0]
    frames = int(r["frames"])
    assert frames >= 320 and frames % P == 0
    L, tx, msg, _ = hostlib.frontend(str(tmp_path), 2.0, frames // P, N, K, code.q, P)
    dec = nb.Decoder(code, nb.METHOD_BP, 30, poll_every=2, layers="greedy", bp=True)
    out, conv, its = dec.decode(L)
    dec.close()
    err_sym, err_bit, _ = hostlib.err_count(str(tmp_path), msg, out)
    print("harness", r, "own", int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum()), "iterations per frame", its.mean())
    assert (r["errFrame"], r["errSym"], r["errBit"]) == (int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum())), r
    assert abs(mean_l - its.mean()) <= 1e-4 * its.mean()
    rc, _, text = _harness(str(tmp_path), "layered")
    assert rc != 0 and "layered schedule is defined for EMS" in text, text
    monkeypatch.setenv("NBL_SCHEDULE", "layered")
    with pytest.raises(RuntimeError):
        hostlib.simulate(str(tmp_path))
