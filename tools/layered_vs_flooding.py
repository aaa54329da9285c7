#!/usr/bin/env python3
"""Flooding against the layered schedule on config 3, end to end with early exit (a number to record, not to assert).

U512.256 GF(256), EMS nm = 32 nc = 3, max_iter 50, early exit with the harness's poll_every (2), batch 4096.  The frames are the
host link chain's own (random message, CRC, encoder, BPSK, AWGN: hostlib.frontend, `batch` lanes, one frame each), the SAME LLRs for
both schedules, resident in HBM.  Per Eb/N0 and schedule: mean iterations per frame, frame errors (decoded word != transmitted
word), ms per iteration (batch time / iterations launched) and frames per second; one warm-up decode, then the median of `repeats`
timed ones (wall clock around a synchronised call).

usage: python tools/layered_vs_flooding.py [batch] [repeats] [EbN0 ...]   -- one JSON line per (Eb/N0, schedule), then a table"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from nbldpc_amd import hostlib  # noqa: E402
from nbldpc_amd.profiles import DEFAULTS  # noqa: E402

CODE = "divsalar.UNBLDPC.512.256.GF.256"
KW = dict(ems_nm=32, ems_nc=3)
MAX_ITER, POLL = 50, 2


def frames(workdir, ebn0, B, code):
    prof = dict(DEFAULTS, gfq=code.q, method=nb.METHOD_EMS, max_iter=MAX_ITER, parallel=B, **KW)
    prof = {k: v for k, v in prof.items() if k not in ("code", "constellation")}
    hostlib.prepare_workdir(workdir, dict(prof, code=CODE), CODE, "BPSK")
    L, tx, _, _ = hostlib.frontend(workdir, ebn0, 1, code.N, code.N - code.M, code.q, B)
    return L, tx


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    points = [float(x) for x in sys.argv[3:]] or [1.0, 1.5, 2.0]
    dev = torch.device("cuda", 0)
    code = nb.Code(CODE)
    out = torch.zeros((B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros(B, dtype=torch.uint8, device=dev)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for ebn0 in points:
        with tempfile.TemporaryDirectory() as tmp:
            L, tx = frames(tmp, ebn0, B, code)
        dL = torch.from_numpy(L).to(dev).contiguous()
        del L
        for sched in ("flooding", "layered"):
            dec = nb.Decoder(code, nb.METHOD_EMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0,
                             layers="greedy" if sched == "layered" else None, **KW)
            times = []
            for k in range(repeats + 1):  # (the first one warms up: workspace, code objects, clocks)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), st)
                torch.cuda.synchronize()
                if k:
                    times.append(time.perf_counter() - t0)
            _, launches = dec.last_timing()
            dt = statistics.median(times)
            ferr = int((out.cpu().numpy() != tx).any(axis=1).sum())
            row = dict(ebn0=ebn0, schedule=sched, batch=B, n_layers=(int(dec.layers.max()) + 1 if sched == "layered" else 1),
                       iterations_per_frame=float(its.double().mean().item()), frame_errors=ferr, not_converged=int(B - conv.sum().item()),
                       iterations_launched=int(launches[1]), ms_per_iteration=dt * 1e3 / max(int(launches[1]), 1), ms_per_batch=dt * 1e3,
                       frames_per_s=B / dt, spread_ms=[min(times) * 1e3, max(times) * 1e3])
            print(json.dumps(row), flush=True)
            rows.append(row)
            dec.close()
        del dL
        torch.cuda.empty_cache()
    print("| Eb/N0 (dB) | schedule | iterations / frame | frame errors / %d | iterations launched | ms / iteration | frames / s |" % B)
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %.1f | %s | %.2f | %d | %d | %.3f | %.0f |" % (r["ebn0"], r["schedule"], r["iterations_per_frame"], r["frame_errors"],
                                                              r["iterations_launched"], r["ms_per_iteration"], r["frames_per_s"]))


if __name__ == "__main__":
    main()
