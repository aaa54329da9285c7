#!/usr/bin/env python3
"""T-EMS decoding (nbl_create_tems_wide) on high-rate codes: random (2, dc)-regular codes with check degrees up to
NBL_TEMS_MAX_CHECK_DEGREE = 32, flooding and damped layered (numbers to record, not to assert).  No file is needed: the graph is drawn
here, by tools/fht_high_rate.py's generator, so a (q, dc, N, seed) names the same code as in tools/fht_high_rate.py and
tools/ems_high_rate.py.

Frames: the all-zero codeword over BPSK / AWGN at the code's rate (N - M) / N, symbol LLRs formed on the device, resident in HBM,
the same frames for every decoder.  Per Eb/N0 point and decoder, over steps x batch frames:
  frame errors (decoded word != 0) and frames that did not converge;
  mean iterations per frame and frames per second with early exit (poll_every 2, max_iter 50);
  codewords per second at 10 fixed iterations (fixed_iters = 1: every launch of every iteration runs on every frame).
Printed once: the bytes of LDS of one check's workgroup and the workgroups per CU they allow (160 KB of LDS per CU).
On a code inside nbl_create's envelope (dc <= 8 and log2(q) dc <= 32) the decoders run as nbl_create / nbl_create_layered_ex makes them;
--force-wide adds the same decoders under nbl_debug_force_generic(dec, 3) (the workgroup-per-check programme of
nbl_cn_tems_wide_core.h), and --general the flooding decoder under switch 1 (the one-wave-per-check general kernel, nbl_cn_tems_core.h),
on the same frames.
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call.

usage: python tools/tems_high_rate.py q dc N [--nr NR] [--nc NC] [--batch B] [--steps S] [--seed X] [--force-wide] [--general] [--fixed-only] [EbN0 ...]
-- one JSON line per (Eb/N0, decoder), then a table"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from fht_high_rate import FIXED, MAX_ITER, POLL, force, llr_zero, regular_code, timed  # noqa: E402


def lds_bytes(q, maxdc, nr, nc):
    fn = nb.load_library().nbl_debug_tems_wide_lds_bytes
    fn.restype, fn.argtypes = C.c_uint64, [C.c_int32] * 4
    return int(fn(q, maxdc, nr, nc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nr", type=int, default=2)
    ap.add_argument("--nc", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--force-wide", action="store_true")
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("rest", nargs="*")
    a = ap.parse_intermixed_args()
    q, dc, N = (int(x) for x in a.rest[:3])
    points = [float(x) for x in a.rest[3:]] or [4.0, 5.0, 6.0]
    code, tag = regular_code(q, dc, N, a.seed), f"(2,{dc})-regular GF({q}) N={N} nr={a.nr} nc={a.nc}"
    B, steps = a.batch, a.steps
    tems = dict(tems_nr=a.nr, tems_nc=a.nc)
    runs = [("tems flooding", dict(), 0), ("tems layered", dict(layers="greedy"), 0)]
    if dc <= 8 and (q.bit_length() - 1) * dc <= 32:
        if a.general:
            runs.append(("tems flooding (general kernel)", dict(), 1))
        if a.force_wide:
            runs += [("tems flooding (forced wide)", dict(), 3), ("tems layered (forced wide)", dict(layers="greedy"), 3)]
    lds = lds_bytes(q, dc, a.nr, a.nc)
    print(json.dumps(dict(code=tag, lds_bytes_per_check=lds, workgroups_per_cu=min(160 * 1024 // lds, 32), waves_per_workgroup=max(1, q // 64))), flush=True)
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
        for label, kw, fg in runs:
            row = dict(code=tag, rate=(N - code.M) / N, check_degree=dc, ebn0=ebn0, decoder=label, batch=B, steps=steps, frames=B * steps)
            if not a.fixed_only:
                dec = nb.Decoder(code, nb.METHOD_TEMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0, tems_wide=True, **tems, **kw)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                row.update(frame_errors=int((out != 0).any(dim=2).sum().item()), not_converged=int(B * steps - conv.sum().item()),
                           iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt)
            dec = nb.Decoder(code, nb.METHOD_TEMS, FIXED, fixed_iters=1, max_batch=B, device=0, tems_wide=True, **tems, **kw)
            force(dec, fg)
            dt = timed(dec, dL, B, out, conv, its, st)
            dec.close()
            row.update(fixed_iterations=FIXED, codewords_per_s_fixed=B * steps / dt)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("%s, rate %.3f, batch %d x %d steps, %d B of LDS per check" % (tag, (N - code.M) / N, B, steps, lds))
    print("| Eb/N0 (dB) | decoder | frame errors / %d | not converged | iterations / frame | frames / s | codewords / s at %d fixed iterations |" % (B * steps, FIXED))
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.2f | %s | %s | %s | %s | %s | %.0f |" % (r["ebn0"], r["decoder"], r.get("frame_errors", "-"), r.get("not_converged", "-"),
                                                          "%.2f" % r["iterations_per_frame"] if "iterations_per_frame" in r else "-",
                                                          "%.0f" % r["frames_per_s"] if "frames_per_s" in r else "-", r["codewords_per_s_fixed"]))


if __name__ == "__main__":
    main()
