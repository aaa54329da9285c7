"""Basic-set T-EMS (decode method 7) on the GPU (nbldpc_amd/csrc/nbl_cn_bstems.hip): against the compiled reference's fixtures and FER
lines, and against the CANONICAL mode of the CPU checker tests/bstems_check.cpp (bit for bit) at scale, on a synthetic grid of
fields and (nm, nc), and across batch shapes."""
import glob
import json
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from nbldpc_amd import datafiles as df
from conftest import GOLD, load_golden
from bstems_util import CANONICAL, bs_kwargs, build_checker, ring_code, run_checker

pytestmark = pytest.mark.gpu

SETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "bstems_*.npz")))
ANCHORS = json.load(open(os.path.join(GOLD, "fer_anchors_bstems.json")))
LLR_TOL = 1e-9


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bstems"))


def _decoder(code, max_iter, kw, **extra):
    return nb.Decoder(code, nb.METHOD_BS_TEMS, max_iter, **kw, **extra)


@pytest.mark.parametrize("name", SETS)
def test_fixture_outputs_equal_reference(name):
    g, meta = load_golden(name)
    kw = bs_kwargs(meta["profile"])
    code = nb.Code(meta["code"])
    for k, it in enumerate(g["iters"]):
        dec = _decoder(code, int(it), kw)
        out, conv, iters = dec.decode(g["L_ch"])
        dec.close()
        assert np.array_equal(out, g["out"][k]), (name, int(it))
        assert np.array_equal(conv, g["ret"][k]) and np.array_equal(conv, g["syn_ok"][k]), (name, int(it))
        assert ((iters <= it) & ((conv == 0) | (iters >= 1))).all()


@pytest.mark.parametrize("name", SETS)
def test_fixture_state_equals_canonical_checker_and_reference(checker, name):
    g, meta = load_golden(name)
    kw = bs_kwargs(meta["profile"])
    code = nb.Code(meta["code"])
    L = g["L_ch"]
    lanes = [int(b) for b in g["state_lanes"]]
    for k, it in enumerate(g["state_iters"]):
        dec = _decoder(code, int(it), kw)
        dec.record_state(True)
        _, conv, iters = dec.decode(L)
        _, c_ret, c_it, st = run_checker(checker, code, L, int(it), CANONICAL, **kw, state=lanes)
        for j, b in enumerate(lanes):
            P, V, Cc = dec.read_state(b)
            cP, cV, cC = st[b]
            # (v2c of a codeword that converged at iteration >= 2: include/nbldpc.h, nbl_read_state)
            v_ok = not (conv[b] and iters[b] >= 2)
            assert np.array_equal(P, cP) and np.array_equal(Cc, cC) and (not v_ok or np.array_equal(V, cV)), (name, int(it), b)
            for a, ref, use in ((P, g["st_post"][k, j], True), (V, g["st_v2c"][k, j], v_ok), (Cc, g["st_c2v"][k, j], True)):
                if use:
                    assert np.max(np.abs(a - ref)) <= LLR_TOL * max(1.0, np.max(np.abs(ref))), (name, int(it), b)
        assert np.array_equal(conv, c_ret) and np.array_equal(iters, c_it)
        dec.close()


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_fer_matches_reference(tmp_path, name):
    from nbldpc_amd import hostlib
    a = ANCHORS[name]
    hostlib.prepare_workdir(str(tmp_path), a["profile"], a["code"], a["constellation"])
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == len(a["points"])
    for got, ref in zip(rows, a["points"]):
        for k in ("EbN0", "frames", "errFrame", "errSym", "errBit", "U_errFrame", "FER", "SER", "BER"):
            assert got[k] == ref[k], (name, k, got, ref)


@pytest.mark.parametrize("device_demod,device_noise", [("1", "0"), ("0", "0")])
def test_fer_with_host_side_front_end(tmp_path, monkeypatch, device_demod, device_noise):
    """The default runs (above) form noise and L_ch on the device; the host-side channel and demodulator give the same counts."""
    from nbldpc_amd import hostlib
    monkeypatch.setenv("NBL_DEVICE_DEMOD", device_demod)
    monkeypatch.setenv("NBL_DEVICE_NOISE", device_noise)
    for name in ("bstems_bds_p4", "bstems_gf256_u128_p8"):
        a = ANCHORS[name]
        hostlib.prepare_workdir(str(tmp_path), a["profile"], a["code"], a["constellation"])
        rows = hostlib.simulate(str(tmp_path))
        for got, ref in zip(rows, a["points"]):
            for k in ("frames", "errFrame", "errSym", "errBit", "U_errFrame"):
                assert got[k] == ref[k], (name, k, got, ref)


def test_sim_binary_prints_bstems_banner(tmp_path):
    import subprocess
    from nbldpc_amd import hostlib
    a = ANCHORS["bstems_gf256_u128_p8"]
    hostlib.prepare_workdir(str(tmp_path), dict(a["profile"], min_sim_cycle=16, snr_begin=3.0, snr_stop=3.0), a["code"], a["constellation"])
    out = subprocess.run([hostlib.SIM_BIN], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Algorithm: BS_TEMS_DECODE\tBS_TEMS_Nm: 8\tBS_TEMS_Nc: 3" in out.stdout
    assert "EbN0\tError\tCRCmiss\tBER" in out.stdout


def _frames(tmp_path, code_name, B, ebn0, seed, **kw):
    from nbldpc_amd import hostlib
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=df.codes()[code_name]["q"], code=code_name, method=7, max_iter=50, parallel=B,
                                                constellation="BPSK", random_msg=1, seed=seed, **kw), code_name, "BPSK")
    c = df.codes()[code_name]
    L, _, _, _ = hostlib.frontend(str(tmp_path), ebn0, 1, c["N"], c["N"] - c["M"], c["q"], B)
    return L


@pytest.mark.parametrize("label,code_name,B,ebn0,iters,nm,nc,fixed", [
    ("gf256_u512_fixed50", "divsalar.UNBLDPC.512.256.GF.256", 256, 2.0, 50, 8, 3, 1),
    ("gf16_u512_early_exit", "divsalar.UNBLDPC.512.256.GF.16", 512, 1.75, 20, 4, 2, 0),
])
def test_harness_frames_at_scale_vs_canonical_checker(tmp_path, checker, label, code_name, B, ebn0, iters, nm, nc, fixed):
    L = _frames(tmp_path, code_name, B, ebn0, 211)
    code = nb.Code(code_name)
    kw = dict(bs_nm=nm, bs_nc=nc, bs_factor=1.0, bs_offset=0.0)
    dec = _decoder(code, iters, kw, fixed_iters=fixed, poll_every=0 if fixed else 2)
    dec.record_state(True)
    out, conv, its = dec.decode(L)
    # state sample: converged codewords (past convergence in fixed-iteration mode) and some that never converge
    sample = sorted(set(np.flatnonzero(conv)[:3].tolist() + np.flatnonzero(conv == 0)[:2].tolist()))
    c_out, c_ret, c_it, st = run_checker(checker, code, L, iters, CANONICAL, nm, nc, fixed_iters=fixed, state=sample)
    assert 0 < conv.sum() < B, (label, int(conv.sum()))
    assert np.array_equal(conv, c_ret) and np.array_equal(its, c_it) and np.array_equal(out, c_out), label
    for b in sample:
        P, V, Cc = dec.read_state(b)
        cP, cV, cC = st[b]
        assert np.array_equal(P, cP) and np.array_equal(Cc, cC), (label, b)
        if fixed or not conv[b] or its[b] < 2:
            assert np.array_equal(V, cV), (label, b)
    dec.close()


GRID = [(q, nm, nc) for q in (4, 8, 32, 128) for nm in sorted({1, min(q - 1, 16)} | {n for n in (2, 3, 5, 7, 12) if n < q})
        for nc in range(0, 5)]


@pytest.mark.parametrize("q", [4, 8, 32, 128])
def test_synthetic_grid_vs_canonical_checker(checker, q):
    """nm < p, = p and > p, nc = 0 .. 4, on (2, 4)-regular ring codes; fixed iterations so that every codeword runs the whole way."""
    rng = np.random.default_rng(q)
    code = ring_code(q, 8, 4)
    L = rng.normal(0.0, 2.0, size=(6, code.N, q - 1))
    L[0] = np.round(L[0])  # integer LLRs: equal configuration costs
    for qq, nm, nc in GRID:
        if qq != q:
            continue
        kw = dict(bs_nm=nm, bs_nc=nc, bs_factor=1.0 if nc % 2 else 1.25, bs_offset=0.0 if nc % 2 else 0.1)
        dec = _decoder(code, 4, kw, fixed_iters=1)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        c_out, c_ret, c_it, st = run_checker(checker, code, L, 4, CANONICAL, fixed_iters=1, state=range(6), **kw)
        assert np.array_equal(out, c_out) and np.array_equal(conv, c_ret) and np.array_equal(its, c_it), (q, nm, nc)
        for b in range(6):
            for a, c in zip(dec.read_state(b), st[b]):
                assert np.array_equal(a, c), (q, nm, nc, b)
        dec.close()


def test_batch_shape_independence():
    """B = 1, 7, 64, 4096 on the same frames, host buffers and device pointers: every codeword decodes alike."""
    import torch
    g, meta = load_golden("bstems_gf16_u128")
    kw = bs_kwargs(meta["profile"])
    code = nb.Code(meta["code"])
    base = g["L_ch"]
    L = np.concatenate([base * (1.0 + 0.01 * k) for k in range(4096 // base.shape[0])])
    dec = _decoder(code, 20, kw, poll_every=2)
    ref = dec.decode(L)
    for B in (1, 7, 64, 4096):
        got = dec.decode(L[:B])
        for a, r in zip(got, ref):
            assert np.array_equal(a, r[:B]), B
        dL = torch.from_numpy(np.ascontiguousarray(L[:B])).cuda()
        out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
        conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
        its = torch.zeros(B, dtype=torch.int32, device="cuda")
        dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for a, r in zip((out, conv, its), ref):
            assert np.array_equal(a.cpu().numpy(), r[:B]), ("device", B)
    dec.close()
    assert 0 < ref[1].sum() < 4096
