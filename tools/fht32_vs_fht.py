#!/usr/bin/env python3
"""FP64 FHT decoding (nbl_create_fht) against single-precision FHT decoding (nbl_create_fht32), flooding and layered, on the SAME
frames (numbers to record, not to assert).  Modelled on tools/fht_vs_exact.py: the same shapes, grids, frames and timing, so the FP64
columns can be checked against that tool's.

--shape cfg5 (default): config 5's shape, C512.256 GF(256) over 256-QAM, max_iter 100, batch 2048, Eb/N0 2.8 / 3.4 / 4.0 dB.
--shape bds64: BDS576.288 GF(64) over BPSK, max_iter 50, batch 4096, Eb/N0 1.0 / 1.5 / 2.0 dB.
Per Eb/N0 point and decoder -- fht flooding, fht32 flooding, fht layered, fht32 layered -- over steps x batch frames:
  frame errors (decoded word != transmitted word), frames that did not converge, frames whose decoded word differs from the FP64
      decoder's of the same schedule;
  mean iterations per frame and frames per second with early exit (poll_every 2, as the harness);
  codewords per second at FIXED fixed iterations, REPEATS times per decoder with the two precisions alternating (fht, fht32, fht, ...
      then the reverse order), minimum / median / maximum.
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call.

usage: python tools/fht32_vs_fht.py [--shape cfg5|bds64] [batch] [steps] [EbN0 ...]
-- one JSON line per (Eb/N0, decoder), then a table"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from fht_vs_exact import SHAPES, POLL, FIXED, frames, timed  # noqa: E402

SCHEDULES = (("flooding", dict()), ("layered", dict(layers="greedy")))
KINDS = (("fht", dict(fht=True)), ("fht32", dict(fht32=True)))
REPEATS = 3  # pairs in each order


def main():
    argv = sys.argv[1:]
    shape = "cfg5"
    if argv and argv[0] == "--shape":
        shape, argv = argv[1], argv[2:]
    name, cons, nqam, random_msg, max_iter, batch, default_points = SHAPES[shape]
    B = int(argv[0]) if len(argv) > 0 else batch
    steps = int(argv[1]) if len(argv) > 1 else 2
    points = [float(x) for x in argv[2:]] or default_points
    dev = torch.device("cuda", 0)
    code = nb.Code(name)
    out = torch.zeros((steps, B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros((steps, B), dtype=torch.uint8, device=dev)
    its = torch.zeros((steps, B), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for ebn0 in points:
        with tempfile.TemporaryDirectory() as tmp:
            L, tx = frames(tmp, ebn0, B, steps, code, name, cons, nqam, random_msg, max_iter)
        dL = torch.from_numpy(L).to(dev).contiguous()
        del L
        for sched, skw in SCHEDULES:
            words = {}
            point = {}
            for kind, kkw in KINDS:
                dec = nb.Decoder(code, nb.METHOD_BP, max_iter, poll_every=POLL, max_batch=B, device=0, **skw, **kkw)
                dt = timed(dec, dL, B, out, conv, its, st, steps)
                dec.close()
                words[kind] = out.cpu().numpy().copy()
                point[kind] = dict(shape=shape, ebn0=ebn0, decoder=f"{kind} {sched}", batch=B, steps=steps, frames=B * steps,
                                   frame_errors=int((words[kind] != tx).any(axis=2).sum()), not_converged=int(B * steps - conv.sum().item()),
                                   iterations_per_frame=float(its.double().mean().item()), frames_per_s=B * steps / dt,
                                   words_differing_from_fht=int((words[kind] != words["fht"]).any(axis=2).sum()))
            # fixed iterations: the two precisions alternate on the one device, REPEATS pairs in each order
            fixed = {kind: nb.Decoder(code, nb.METHOD_BP, FIXED, fixed_iters=1, max_batch=B, device=0, **skw, **kkw) for kind, kkw in KINDS}
            rates = {kind: [] for kind, _ in KINDS}
            for order in (("fht", "fht32"), ("fht32", "fht")):
                for _ in range(REPEATS):
                    for kind in order:
                        rates[kind].append(B * steps / timed(fixed[kind], dL, B, out, conv, its, st, steps))
            for kind, _ in KINDS:
                fixed[kind].close()
                r = sorted(rates[kind])
                point[kind].update(fixed_iterations=FIXED, codewords_per_s_fixed=float(np.median(r)), codewords_per_s_fixed_min=r[0],
                                   codewords_per_s_fixed_max=r[-1], runs=len(r))
                print(json.dumps(point[kind]), flush=True)
                rows.append(point[kind])
        del dL
        torch.cuda.empty_cache()
    print("| Eb/N0 (dB) | decoder | frame errors / %d | not converged | words != fht | iterations / frame | frames / s | codewords / s at %d fixed "
          "iterations: median (min .. max of %d) |" % (B * steps, FIXED, 2 * REPEATS))
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.1f | %s | %d | %d | %d | %.2f | %.0f | %.0f (%.0f .. %.0f) |" % (
            r["ebn0"], r["decoder"], r["frame_errors"], r["not_converged"], r["words_differing_from_fht"], r["iterations_per_frame"],
            r["frames_per_s"], r["codewords_per_s_fixed"], r["codewords_per_s_fixed_min"], r["codewords_per_s_fixed_max"]))


if __name__ == "__main__":
    main()
