#!/usr/bin/env python3
"""Exact log-QSPA (nbl_create_bp_wide) against FHT sum-product decoding (nbl_create_fht) on high-rate codes: random (2, dc)-regular codes
with check degrees up to 32, flooding and layered, ON THE SAME FRAMES (numbers to record, not to assert).  What the floor of the FHT
check node costs at high rate, and what the exact check node costs in time.  No file is needed: the graph is drawn here
(tools/fht_high_rate.py).

Frames: the all-zero codeword over BPSK / AWGN at the code's rate (N - M) / N, symbol LLRs formed on the device, resident in HBM.
Per Eb/N0 point and decoder, over steps x batch frames:
  frame errors (decoded word != 0) and frames that did not converge;
  mean iterations per frame and frames per second with early exit (poll_every 2, max_iter 50);
  codewords per second at 10 fixed iterations (fixed_iters = 1: every launch of every iteration runs on every frame).
On a shape with dc <= 8 the exact decoders run twice: under nbl_debug_force_generic(dec, 1) (the general programme of
nbl_cn_bp_core.h, one wave per check) and under switch 3 (the wide programme of nbl_cn_bp_wide_core.h), on the same frames; the
decoder as created (the fused kernels where they apply) is what tools/fht_vs_exact.py measures.
--fixed-only leaves the early-exit runs out.
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call.

usage: python tools/bp_high_rate.py q dc N [--batch B] [--steps S] [--seed X] [--fixed-only] [EbN0 ...]
-- one JSON line per (Eb/N0, decoder), then a table"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from fht_high_rate import FIXED, MAX_ITER, POLL, force, llr_zero, regular_code, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("rest", nargs="*")
    a = ap.parse_intermixed_args()
    q, dc, N = (int(x) for x in a.rest[:3])
    code, tag = regular_code(q, dc, N, a.seed), f"(2,{dc})-regular GF({q}) N={N}"
    points = [float(x) for x in a.rest[3:]] or [4.0, 5.0, 6.0]
    B, steps = a.batch, a.steps
    exact = (("", 0),) if dc > 8 else ((" (general)", 1), (" (forced wide)", 3))
    decoders = [("exact flooding" + s, dict(bp_wide=True), fg) for s, fg in exact] + \
               [("exact layered" + s, dict(layers="greedy", bp_wide=True), fg) for s, fg in exact] + \
               [("fht flooding", dict(fht=True), 0), ("fht layered", dict(layers="greedy", fht=True), 0)]
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    out = torch.zeros((steps, B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros((steps, B), dtype=torch.uint8, device=dev)
    its = torch.zeros((steps, B), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for ebn0 in points:
        dL = [llr_zero(code, B, ebn0, dev, gen) for _ in range(steps)]
        for label, kw, fg in decoders:
            row = dict(code=tag, rate=(N - code.M) / N, check_degree=dc, ebn0=ebn0, decoder=label, batch=B, steps=steps, frames=B * steps)
            if not a.fixed_only:
                dec = nb.Decoder(code, nb.METHOD_BP, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **kw)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                row.update(frame_errors=int((out != 0).any(dim=2).sum().item()), not_converged=int(B * steps - conv.sum().item()),
                           iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt)
            dec = nb.Decoder(code, nb.METHOD_BP, FIXED, fixed_iters=1, max_batch=B, device=0, **kw)
            force(dec, fg)
            dt = timed(dec, dL, B, out, conv, its, st)
            dec.close()
            row.update(fixed_iterations=FIXED, codewords_per_s_fixed=B * steps / dt)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("%s, rate %.3f, batch %d x %d steps" % (tag, (N - code.M) / N, B, steps))
    print("| Eb/N0 (dB) | decoder | frame errors / %d | not converged | iterations / frame | frames / s | codewords / s at %d fixed iterations |" % (B * steps, FIXED))
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        if a.fixed_only:
            print("| %.2f | %s | | | | | %.0f |" % (r["ebn0"], r["decoder"], r["codewords_per_s_fixed"]))
        else:
            print("| %.2f | %s | %d | %d | %.2f | %.0f | %.0f |" % (r["ebn0"], r["decoder"], r["frame_errors"], r["not_converged"], r["iterations_per_frame"],
                                                                  r["frames_per_s"], r["codewords_per_s_fixed"]))


if __name__ == "__main__":
    main()
