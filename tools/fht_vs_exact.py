#!/usr/bin/env python3
"""Exact log-QSPA against FHT sum-product decoding (nbl_create_fht), flooding and layered, on the SAME frames (numbers to record, not
to assert).

--shape cfg5 (default): config 5's shape, C512.256 GF(256) over 256-QAM, max_iter 100, batch 2048, Eb/N0 2.8 / 3.4 / 4.0 dB.  Its
frames carry the all-zero message (tools/layered_vs_flooding.py says why).
--shape bds64: BDS576.288 GF(64) over BPSK, max_iter 50, batch 4096, Eb/N0 1.0 / 1.5 / 2.0 dB.
The frames are the host link chain's own (hostlib.frontend, `batch` lanes, `steps` frames each), the same LLRs for all four decoders,
resident in HBM.  Per Eb/N0 point and decoder -- exact flooding (nbl_create: the fused kernels), exact layered (nbl_create_layered_bp),
FHT flooding, FHT layered -- over steps x batch frames:
  frame errors (decoded word != transmitted word) and frames that did not converge;
  mean iterations per frame and frames per second with early exit (poll_every 2, as the harness);
  codewords per second at fixed iterations (fixed_iters = 1, FIXED iterations: every launch of every iteration runs on every frame).
Timing: one warm-up decode of the first step, then every step timed by wall clock around a synchronised call; the figure is total frames
over total time.

usage: python tools/fht_vs_exact.py [--shape cfg5|bds64] [batch] [steps] [EbN0 ...]
-- one JSON line per (Eb/N0, decoder), then a table"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402,F401
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from nbldpc_amd import hostlib  # noqa: E402
from nbldpc_amd.profiles import DEFAULTS  # noqa: E402

# shape -> (code, constellation, modulation order, random message, max_iter, default batch, default Eb/N0 points)
SHAPES = {"cfg5": ("divsalar.CNBLDPC.512.256.GF.256", "GRAY_256QAM", 256, 0, 100, 2048, [2.8, 3.4, 4.0]),
          "bds64": ("BDS.576.288.GF.64", "BPSK", 2, 1, 50, 4096, [1.0, 1.5, 2.0])}
DECODERS = (("exact flooding", dict()), ("exact layered", dict(layers="greedy", bp=True)),
            ("fht flooding", dict(fht=True)), ("fht layered", dict(layers="greedy", fht=True)))
POLL = 2
FIXED = 10


def frames(workdir, ebn0, B, steps, code, name, cons, nqam, random_msg, max_iter):
    prof = dict(DEFAULTS, gfq=code.q, method=nb.METHOD_BP, max_iter=max_iter, parallel=B, nqam=nqam, random_msg=random_msg)
    prof = {k: v for k, v in prof.items() if k not in ("code", "constellation")}
    hostlib.prepare_workdir(workdir, dict(prof, code=name), name, cons)
    L, tx, _, _ = hostlib.frontend(workdir, ebn0, steps, code.N, code.N - code.M, code.q, B)
    return L.reshape(steps, B, code.N, code.q - 1), tx.reshape(steps, B, code.N)


def timed(dec, dL, B, out, conv, its, st, steps):
    """seconds for all `steps` decodes, after one warm-up decode of step 0 (workspace, code objects, clocks)"""
    total = 0.0
    for n, k in enumerate([0] + list(range(steps))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_device(dL[k].data_ptr(), B, out[k].data_ptr(), conv[k].data_ptr(), its[k].data_ptr(), st)
        torch.cuda.synchronize()
        if n:
            total += time.perf_counter() - t0
    return total


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
        for label, kw in DECODERS:
            dec = nb.Decoder(code, nb.METHOD_BP, max_iter, poll_every=POLL, max_batch=B, device=0, **kw)
            dt = timed(dec, dL, B, out, conv, its, st, steps)
            dec.close()
            ferr = int((out.cpu().numpy() != tx).any(axis=2).sum())
            row = dict(shape=shape, ebn0=ebn0, decoder=label, batch=B, steps=steps, frames=B * steps, frame_errors=ferr,
                       not_converged=int(B * steps - conv.sum().item()), iterations_per_frame=float(its.double().mean().item()),
                       frames_per_s=B * steps / dt)
            dec = nb.Decoder(code, nb.METHOD_BP, FIXED, fixed_iters=1, max_batch=B, device=0, **kw)
            dt = timed(dec, dL, B, out, conv, its, st, steps)
            dec.close()
            row.update(fixed_iterations=FIXED, codewords_per_s_fixed=B * steps / dt)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del dL
        torch.cuda.empty_cache()
    print("| Eb/N0 (dB) | decoder | frame errors / %d | not converged | iterations / frame | frames / s | codewords / s at %d fixed iterations |" % (B * steps, FIXED))
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.1f | %s | %d | %d | %.2f | %.0f | %.0f |" % (r["ebn0"], r["decoder"], r["frame_errors"], r["not_converged"],
                                                              r["iterations_per_frame"], r["frames_per_s"], r["codewords_per_s_fixed"]))


if __name__ == "__main__":
    main()
