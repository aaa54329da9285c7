#!/usr/bin/env python3
"""FHT sum-product decoding (nbl_create_fht) on high-rate codes: random (2, dc)-regular codes with check degrees up to
NBL_FHT_MAX_CHECK_DEGREE = 32, flooding and layered (numbers to record, not to assert).  No file is needed: the graph is drawn here.

Frames: the all-zero codeword over BPSK / AWGN at the code's rate (N - M) / N, symbol LLRs formed on the device, resident in HBM,
the same frames for every decoder.  Per Eb/N0 point and decoder, over steps x batch frames:
  frame errors (decoded word != 0) and frames that did not converge;
  mean iterations per frame and frames per second with early exit (poll_every 2, max_iter 50);
  codewords per second at 10 fixed iterations (fixed_iters = 1: every launch of every iteration runs on every frame) and the share of
  the 8 TB/s algorithmic-bytes roofline that is (tools/bench_config.py: 8 (q - 1) (N + 5 E) bytes per codeword and iteration for a
  damped method, plus the input and the output).
On a shape with dc <= 8 every decoder runs twice: as created (the register programme of nbl_cn_fht_core.h) and under
nbl_debug_force_generic(dec, 3) (the wide programme of nbl_cn_fht_wide_core.h), on the same frames.
--code NAME takes a shipped code instead of a drawn one (e.g. config 5's shape, divsalar.CNBLDPC.512.256.GF.256).
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call.

usage: python tools/fht_high_rate.py [--code NAME | q dc N] [--batch B] [--steps S] [--seed X] [EbN0 ...]
-- one JSON line per (Eb/N0, decoder), then a table"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402

POLL, FIXED, MAX_ITER = 2, 10, 50


def regular_code(q, dc, N, seed):
    """A random (2, dc)-regular graph: M = 2 N / dc checks; the 2 N sockets of the checks are shuffled and dealt to the variables two
    by two; a variable dealt the same check twice swaps a socket with another variable until none is left.  Non-zero coefficients from
    the seed."""
    assert (2 * N) % dc == 0 and 2 * N // dc > 2
    M = 2 * N // dc
    rng = np.random.default_rng(seed)
    s = np.repeat(np.arange(M), dc)
    rng.shuffle(s)
    s = s.reshape(N, 2)
    for _ in range(100 * N):
        bad = np.flatnonzero(s[:, 0] == s[:, 1])
        if not len(bad):
            break
        n, o = int(bad[0]), int(rng.integers(N))
        s[n, 1], s[o, 1] = s[o, 1], s[n, 1]
    assert not np.any(s[:, 0] == s[:, 1])
    var_rows = [[(int(m) + 1, int(rng.integers(1, q))) for m in sorted(r)] for r in s]
    chk_rows = [[] for _ in range(M)]
    for n, r in enumerate(var_rows):
        for m1, h in r:
            chk_rows[m1 - 1].append((n + 1, h))
    code = nb.Code(spec=dict(N=N, M=M, q=q, var_rows=var_rows, chk_rows=chk_rows))
    assert set(code.chk_deg.tolist()) == {dc} and set(code.var_deg.tolist()) == {2}
    return code


def llr_zero(code, B, ebn0_db, dev, gen):
    """[B][N][q-1] symbol LLRs of the all-zero codeword over BPSK / AWGN at the code's rate"""
    p = code.q.bit_length() - 1
    rate = (code.N - code.M) / code.N
    sigma = 1.0 / np.sqrt(2 * rate * 10 ** (ebn0_db / 10.0))
    bit = -2.0 * (1.0 + sigma * torch.randn((B, code.N, p), dtype=torch.float64, device=dev, generator=gen)) / sigma ** 2
    a = torch.arange(1, code.q, device=dev)
    mask = ((a[:, None] >> torch.arange(p, device=dev)[None, :]) & 1).to(torch.float64)
    return (bit @ mask.T).contiguous()


def force(dec, on):
    dec.lib.nbl_debug_force_generic.argtypes = [C.c_void_p, C.c_int32]
    assert dec.lib.nbl_debug_force_generic(dec.h, int(on)) == 0


def timed(dec, dL, B, out, conv, its, st):
    """seconds for one decode of every step, after one warm-up decode of step 0 (workspace, code objects, clocks)"""
    total = 0.0
    for n, k in enumerate([0] + list(range(len(dL)))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_device(dL[k].data_ptr(), B, out[k].data_ptr(), conv[k].data_ptr(), its[k].data_ptr(), st)
        torch.cuda.synchronize()
        if n:
            total += time.perf_counter() - t0
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("rest", nargs="*")
    a = ap.parse_intermixed_args()
    rest = list(a.rest)
    if a.code:
        code, tag = nb.Code(a.code), a.code
    else:
        q, dc, N = (int(x) for x in rest[:3])
        rest = rest[3:]
        code, tag = regular_code(q, dc, N, a.seed), f"(2,{dc})-regular GF({q}) N={N}"
    points = [float(x) for x in rest] or [4.0, 5.0, 6.0]
    B, steps = a.batch, a.steps
    maxdc = int(code.chk_deg.max())
    layouts = (("", 0),) if maxdc > 8 else ((" (register)", 0), (" (forced wide)", 3))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    out = torch.zeros((steps, B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros((steps, B), dtype=torch.uint8, device=dev)
    its = torch.zeros((steps, B), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    q, N, E = code.q, code.N, int(code.var_deg.sum())
    bytes_cw = 8 * (q - 1) * N + FIXED * 8 * (q - 1) * (N + 5 * E) + 4 * N + 4
    rows = []
    for ebn0 in points:
        dL = [llr_zero(code, B, ebn0, dev, gen) for _ in range(steps)]
        for label, kw in (("fht flooding", dict(fht=True)), ("fht layered", dict(layers="greedy", fht=True))):
            for suffix, fg in layouts:
                dec = nb.Decoder(code, nb.METHOD_BP, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **kw)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                row = dict(code=tag, rate=(N - code.M) / N, check_degree=maxdc, ebn0=ebn0, decoder=label + suffix, batch=B, steps=steps, frames=B * steps,
                           frame_errors=int((out != 0).any(dim=2).sum().item()), not_converged=int(B * steps - conv.sum().item()),
                           iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt)
                dec = nb.Decoder(code, nb.METHOD_BP, FIXED, fixed_iters=1, max_batch=B, device=0, **kw)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                cws = B * steps / dt
                row.update(fixed_iterations=FIXED, codewords_per_s_fixed=cws, hbm_frac_fixed=cws * bytes_cw / 8e12)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("%s, rate %.3f, batch %d x %d steps" % (tag, (N - code.M) / N, B, steps))
    print("| Eb/N0 (dB) | decoder | frame errors / %d | not converged | iterations / frame | frames / s | codewords / s at %d fixed iterations | of 8 TB/s |" % (B * steps, FIXED))
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.2f | %s | %d | %d | %.2f | %.0f | %.0f | %.1f %% |" % (r["ebn0"], r["decoder"], r["frame_errors"], r["not_converged"], r["iterations_per_frame"],
                                                                        r["frames_per_s"], r["codewords_per_s_fixed"], 100 * r["hbm_frac_fixed"]))


if __name__ == "__main__":
    main()
