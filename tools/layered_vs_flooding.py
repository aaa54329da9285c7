#!/usr/bin/env python3
"""Flooding against the layered schedule, end to end with early exit (a number to record, not to assert).

--method ems (default): config 3's shape, U512.256 GF(256), EMS nm = 32 nc = 3, against nbl_create_layered.
--method tems: config 4's shape, BDS576.288 GF(64), T-EMS nr = 2 nc = 3, against the damped layered schedule (nbl_create_layered_ex
with NBL_LAYERED_DAMPED).
--method bp: config 5's shape, C512.256 GF(256) over 256-QAM, log-QSPA, max_iter 100, against nbl_create_layered_bp (flooding runs the
fused GF(256) kernel, one launch per iteration; layered the general programme, one launch per layer plus decision and syndrome).
Its frames carry the all-zero message (Random Msg 0): with a random message the reference's QAM chain maps transmit and receive bits in
different orders and no frame decodes at any Eb/N0.
--method bp64: BDS576.288 GF(64) over BPSK, log-QSPA, the same comparison.
max_iter 50 unless said otherwise, early exit with the harness's poll_every (2), batch 4096 (2048 for --method bp).  The frames are the
host link chain's own (random message, CRC, encoder, modulation, AWGN: hostlib.frontend, `batch` lanes, one frame each), the SAME LLRs for
both schedules, resident in HBM.  Per Eb/N0 and schedule: mean iterations per frame, frame errors (decoded word != transmitted
word), ms per iteration (batch time / iterations launched) and frames per second; one warm-up decode, then the median of `repeats`
timed ones (wall clock around a synchronised call).

usage: python tools/layered_vs_flooding.py [--method ems|tems|bp|bp64] [batch] [repeats] [EbN0 ...]
-- one JSON line per (Eb/N0, schedule), then a table"""
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

# method switch -> (code, nbl method, its parameters, the layered decoder's extra arguments, its name in the table,
#                   constellation, modulation order, random message, max_iter, default batch, default Eb/N0 points)
SHAPES = {"ems": ("divsalar.UNBLDPC.512.256.GF.256", nb.METHOD_EMS, dict(ems_nm=32, ems_nc=3), dict(layers="greedy"), "layered",
                  "BPSK", 2, 1, 50, 4096, [1.0, 1.5, 2.0]),
          "tems": ("BDS.576.288.GF.64", nb.METHOD_TEMS, dict(tems_nr=2, tems_nc=3), dict(layers="greedy", damped=True), "layered-damped",
                   "BPSK", 2, 1, 50, 4096, [1.0, 1.5, 2.0]),
          "bp": ("divsalar.CNBLDPC.512.256.GF.256", nb.METHOD_BP, dict(), dict(layers="greedy", bp=True), "layered-bp",
                 "GRAY_256QAM", 256, 0, 100, 2048, [2.8, 3.4, 4.0]),
          "bp64": ("BDS.576.288.GF.64", nb.METHOD_BP, dict(), dict(layers="greedy", bp=True), "layered-bp",
                   "BPSK", 2, 1, 50, 4096, [1.0, 1.5, 2.0])}
POLL = 2


def frames(workdir, ebn0, B, code, name, method, kw, cons, nqam, random_msg, max_iter):
    prof = dict(DEFAULTS, gfq=code.q, method=method, max_iter=max_iter, parallel=B, nqam=nqam, random_msg=random_msg, **kw)
    prof = {k: v for k, v in prof.items() if k not in ("code", "constellation")}
    hostlib.prepare_workdir(workdir, dict(prof, code=name), name, cons)
    L, tx, _, _ = hostlib.frontend(workdir, ebn0, 1, code.N, code.N - code.M, code.q, B)
    return L, tx


def main():
    argv = sys.argv[1:]
    which = "ems"
    if argv and argv[0] == "--method":
        which, argv = argv[1], argv[2:]
    name, method, kw, lay_kw, lay_name, cons, nqam, random_msg, MAX_ITER, batch, default_points = SHAPES[which]
    B = int(argv[0]) if len(argv) > 0 else batch
    repeats = int(argv[1]) if len(argv) > 1 else 5
    points = [float(x) for x in argv[2:]] or default_points
    dev = torch.device("cuda", 0)
    code = nb.Code(name)
    out = torch.zeros((B, code.N), dtype=torch.int32, device=dev)
    conv = torch.zeros(B, dtype=torch.uint8, device=dev)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for ebn0 in points:
        with tempfile.TemporaryDirectory() as tmp:
            L, tx = frames(tmp, ebn0, B, code, name, method, kw, cons, nqam, random_msg, MAX_ITER)
        dL = torch.from_numpy(L).to(dev).contiguous()
        del L
        for sched in ("flooding", lay_name):
            dec = nb.Decoder(code, method, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **(lay_kw if sched != "flooding" else {}), **kw)
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
            row = dict(ebn0=ebn0, schedule=sched, batch=B, method=which, n_layers=(int(dec.layers.max()) + 1 if sched != "flooding" else 1),
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
