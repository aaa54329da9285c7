#!/usr/bin/env python3
"""Single-precision FHT decoding for high-rate codes (nbl_create_fht32_wide, check degrees up to NBL_FHT32_MAX_CHECK_DEGREE = 32)
beside FP64 FHT decoding (nbl_create_fht) on the same frames, flooding and layered (numbers to record, not to assert).  The codes, the
frames and the early-exit measurement are those of tools/fht_high_rate.py: random (2, dc)-regular codes, the all-zero codeword over
BPSK / AWGN at the code's rate, symbol LLRs formed on the device.

Per Eb/N0 point, schedule and decoder, over steps x batch frames: frame errors (decoded word != 0), frames that did not converge, mean
iterations per frame and frames per second with early exit (poll_every 2, max_iter 50).
Per schedule, on the frames of the first point: codewords per second at 10 fixed iterations of both decoders, ALTERNATED on the one
device -- three runs FP64 then FP32, three runs FP32 then FP64; mean and range of the six runs of each, and the ratio of the means.
On a shape with dc <= 8 the FP32 decoder runs twice: as created (the register programme of nbl_cn_fht32_core.h, what nbl_create_fht32
makes) and under nbl_debug_force_generic(dec, 3) (the wide programme of nbl_cn_fht32_wide_core.h), which shows what the wide programme
costs where the register programme is the default.
--code NAME takes a shipped code instead of a drawn one (e.g. config 5's shape, divsalar.CNBLDPC.512.256.GF.256).

usage: python tools/fht32_high_rate.py [--code NAME | q dc N] [--batch B] [--steps S] [--seed X] [EbN0 ...]
-- one JSON line per measurement, then two tables"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from fht_high_rate import FIXED, MAX_ITER, POLL, force, llr_zero, regular_code, timed  # noqa: E402

PAIRS = 3   # per order


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
    # (label, Decoder keywords, debug switch)
    kinds = [("fp64", dict(fht=True), 0)] + ([("fp32 wide", dict(fht32_wide=True), 0)] if maxdc > 8 else
                                             [("fp32 (register)", dict(fht32_wide=True), 0), ("fp32 (forced wide)", dict(fht32_wide=True), 3)])
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    out = torch.zeros((steps, B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros((steps, B), dtype=torch.uint8, device=dev)
    its = torch.zeros((steps, B), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    N = code.N
    rows, fixed_rows = [], []
    for n_point, ebn0 in enumerate(points):
        dL = [llr_zero(code, B, ebn0, dev, gen) for _ in range(steps)]
        for sched, lay in (("flooding", {}), ("layered", dict(layers="greedy"))):
            for label, kw, fg in kinds:
                dec = nb.Decoder(code, nb.METHOD_BP, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **kw, **lay)
                force(dec, fg)
                dt = timed(dec, dL, B, out, conv, its, st)
                dec.close()
                row = dict(code=tag, rate=(N - code.M) / N, check_degree=maxdc, ebn0=ebn0, schedule=sched, decoder=label, batch=B, steps=steps, frames=B * steps,
                           frame_errors=int((out != 0).any(dim=2).sum().item()), not_converged=int(B * steps - conv.sum().item()),
                           iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt)
                print(json.dumps(row), flush=True)
                rows.append(row)
            if n_point:
                continue
            # 10 fixed iterations, the decoders alternated: every FP32 variant against FP64, PAIRS runs in each order
            for label, kw, fg in kinds[1:]:
                decs = []
                for k, f in ((kinds[0][1], 0), (kw, fg)):
                    d = nb.Decoder(code, nb.METHOD_BP, FIXED, fixed_iters=1, max_batch=B, device=0, **k, **lay)
                    force(d, f)
                    decs.append(d)
                rates = ([], [])
                for order in ((0, 1),) * PAIRS + ((1, 0),) * PAIRS:
                    for i in order:
                        rates[i].append(B * steps / timed(decs[i], dL, B, out, conv, its, st))
                for d in decs:
                    d.close()
                mean = [sum(r) / len(r) for r in rates]
                row = dict(code=tag, check_degree=maxdc, ebn0=ebn0, schedule=sched, decoder=label, fixed_iterations=FIXED, runs_each=2 * PAIRS,
                           fp64_codewords_per_s=mean[0], fp64_range=[min(rates[0]), max(rates[0])],
                           fp32_codewords_per_s=mean[1], fp32_range=[min(rates[1]), max(rates[1])], ratio=mean[1] / mean[0])
                print(json.dumps(row), flush=True)
                fixed_rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("%s, rate %.3f, batch %d x %d steps" % (tag, (N - code.M) / N, B, steps))
    print("| Eb/N0 (dB) | schedule | decoder | frame errors / %d | not converged | iterations / frame | frames / s |" % (B * steps))
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.2f | %s | %s | %d | %d | %.2f | %.0f |" % (r["ebn0"], r["schedule"], r["decoder"], r["frame_errors"], r["not_converged"], r["iterations_per_frame"],
                                                            r["frames_per_s"]))
    print("| schedule | FP32 decoder | FP64 codewords / s at %d fixed iterations (range of %d) | FP32 (range) | FP32 / FP64 |" % (FIXED, 2 * PAIRS))
    print("|---|---|---|---|---|")
    for r in fixed_rows:
        print("| %s | %s | %.0f (%.0f .. %.0f) | %.0f (%.0f .. %.0f) | %.2f |" % (r["schedule"], r["decoder"], r["fp64_codewords_per_s"], *r["fp64_range"],
                                                                              r["fp32_codewords_per_s"], *r["fp32_range"], r["ratio"]))


if __name__ == "__main__":
    main()
