#!/usr/bin/env python3
"""Min-Max decoding (nbl_create_minmax) beside EMS, exact log-QSPA and FHT sum-product decoding, flooding and layered, ON THE SAME FRAMES
(numbers to record, not to assert).

--shape cfg3 (default): config 3's code, divsalar.UNBLDPC.512.256.GF.256, batch 2048, Eb/N0 2.0 / 2.5 / 3.0 dB, EMS nm 32 nc 3.
--shape bds64: BDS.576.288.GF.64, batch 2048, Eb/N0 1.0 / 1.5 / 2.0 dB, EMS nm 16 nc 3.
--shape hr64: the (2,16)-regular GF(64) N = 1152 code of tools/fht_high_rate.py (seed 1), batch 1024, Eb/N0 3.0 / 3.5 / 4.0 dB, EMS nm 16 nc 3.
Frames: the all-zero codeword over BPSK / AWGN at the code's rate, symbol LLRs formed on the device (tools/fht_high_rate.py), the same
LLRs for every decoder, resident in HBM.  EMS, exact log-QSPA and FHT go through nbl_create_ems_wide, nbl_create_bp_wide and
nbl_create_fht: on a code whose checks have degree 8 or less the first two are the decoders of nbl_create / nbl_create_layered*, fused
kernels included.  "exact .. (wide programme)" is nbl_create_bp_wide under nbl_debug_force_generic(dec, 3), the workgroup-per-check
programme whose storage scheme the Min-Max kernel shares (left out where the code needs that programme anyway).
Per Eb/N0 point and decoder, over steps x batch frames:
  frame errors (decoded word != 0) and frames that did not converge;
  mean iterations per frame and frames per second with early exit (poll_every 2, max_iter 50);
  codewords per second at 10 fixed iterations (fixed_iters = 1: every launch of every iteration runs on every frame).
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call.

usage: python tools/minmax_rate.py [--shape cfg3|bds64|hr64] [--batch B] [--steps S] [--seed X] [--fixed-only] [EbN0 ...]
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

# shape -> (code, EMS parameters, default batch, default Eb/N0 points)
SHAPES = {"cfg3": (lambda seed: nb.Code("divsalar.UNBLDPC.512.256.GF.256"), dict(ems_nm=32, ems_nc=3), 2048, [2.0, 2.5, 3.0]),
          "bds64": (lambda seed: nb.Code("BDS.576.288.GF.64"), dict(ems_nm=16, ems_nc=3), 2048, [1.0, 1.5, 2.0]),
          "hr64": (lambda seed: regular_code(64, 16, 1152, seed), dict(ems_nm=16, ems_nc=3), 1024, [3.0, 3.5, 4.0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg3", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("points", nargs="*", type=float)
    a = ap.parse_intermixed_args()
    make, ems, batch, default_points = SHAPES[a.shape]
    code = make(a.seed)
    B, steps, points = a.batch or batch, a.steps, a.points or default_points
    tag = f"{a.shape}: GF({code.q}) N={code.N} M={code.M}, check degrees {int(code.chk_deg.min())}..{int(code.chk_deg.max())}"
    decoders = []
    for sched, lay in (("flooding", {}), ("layered", dict(layers="greedy"))):
        decoders += [(f"minmax {sched}", nb.METHOD_MINMAX, dict(minmax=True, **lay), 0), (f"ems {sched}", nb.METHOD_EMS, dict(wide=True, **ems, **lay), 0),
                     (f"exact {sched}", nb.METHOD_BP, dict(bp_wide=True, **lay), 0)]
        if code.chk_deg.max() <= 8:
            decoders.append((f"exact {sched} (wide programme)", nb.METHOD_BP, dict(bp_wide=True, **lay), 3))
        decoders.append((f"fht {sched}", nb.METHOD_BP, dict(fht=True, **lay), 0))
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
        for label, method, kw, fg in decoders:
            row = dict(shape=a.shape, code=tag, ebn0=ebn0, decoder=label, batch=B, steps=steps, frames=B * steps)
            if not a.fixed_only:
                dec = nb.Decoder(code, method, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **kw)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                row.update(frame_errors=int((out != 0).any(dim=2).sum().item()), not_converged=int(B * steps - conv.sum().item()),
                           iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt)
            dec = nb.Decoder(code, method, FIXED, fixed_iters=1, max_batch=B, device=0, **kw)
            force(dec, fg)
            dt = timed(dec, dL, B, out, conv, its, st)
            dec.close()
            row.update(fixed_iterations=FIXED, codewords_per_s_fixed=B * steps / dt)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("%s, batch %d x %d steps" % (tag, B, steps))
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
