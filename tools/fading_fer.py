#!/usr/bin/env python3
"""Frame errors over AWGN against Rayleigh fading, with and without iterative demapping (numbers to record in DESIGN.md section 5k,
not to assert).

tools/idd_gain.py's set-up: BDS576.288 GF(64), EMS nm = 16 nc = 3, max_iter 50, early exit (poll_every 2), Gray 16-QAM through a
fixed random bit interleaver; `frames` random-message code words of the host chain (hostlib.frontend) per Eb/N0 point, modulated here.
Three channels, the same noise for all: AWGN (gain-less call), Rayleigh with one gain per sample (coherence 1) and Rayleigh with one
gain per frame (coherence L), the gains complex normals of unit mean power (numpy, seeded) handed to decode_samples_idd(gain=).
Decoded with passes = 1 / 2 / 3 (max-log demodulator, max-log extrinsic).  Per cell: frame errors, iterations per frame (summed over
the passes a frame ran), frames per second of the call (host wall clock, host buffers).

With `demod` as the first argument: device time of ONE demodulator launch with and without gains (nbl_debug_time_demod_csi) on the
samples the device-side channel left in a slot, on this set-up's general demodulator and on the reference-pinned paths (the q-ary shapes
of benchmark configurations 4 and 5 at their batch sizes, and GF(256) BPSK), and the channel's wall time per batch with and without
fading.

usage: python tools/fading_fer.py [frames] [EbN0 ...]     -- one JSON line per channel, then a table
       python tools/fading_fer.py demod [batch] [repeats]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
import nbldpc_amd.datafiles as df  # noqa: E402
from nbldpc_amd import hostlib  # noqa: E402
from nbldpc_amd.profiles import DEFAULTS  # noqa: E402
from idd_gain import CONS, KW, MAX_ITER, NAME, POLL, SEED, modulate  # noqa: E402


def fer_table(argv):
    B = int(argv[0]) if len(argv) > 0 else 4096
    ebn0s = [float(x) for x in argv[1:]] or [3.5, 4.5, 5.5, 6.5, 8.0, 12.0, 16.0]   # AWGN falls between 2.5 and 4.5 dB, coherence 1 between 4.5 and 8
    code = nb.Code(NAME)
    N, q, K = code.N, code.q, code.N - code.M
    p = q.bit_length() - 1
    points = np.array([[x[1], x[2]] for x in sorted(df.constellation(CONS))], dtype=np.float64)
    m = 4
    L = N * p // m
    src = np.random.default_rng(SEED).permutation(N * p).astype(np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        prof = {k: v for k, v in dict(DEFAULTS, gfq=q, method=2, max_iter=MAX_ITER, parallel=B, **KW).items() if k not in ("code", "constellation")}
        hostlib.prepare_workdir(tmp, dict(prof, code=NAME, random_msg=1), NAME, "BPSK")
        _, tx, msg, _ = hostlib.frontend(tmp, 5.0, 1, N, K, q, B)
    idx = modulate(tx, p, src, m, L)
    noise = np.random.default_rng(SEED + 1).standard_normal((B, L, 2))
    h = np.random.default_rng(SEED + 2).standard_normal((B, L, 2)) * np.sqrt(0.5)
    channels = (("awgn", None), ("rayleigh, coherence 1", h), ("rayleigh, coherence L", np.ascontiguousarray(np.broadcast_to(h[:, :1], h.shape))))
    dec = nb.Decoder(code, nb.METHOD_EMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **KW)
    dec.set_demodulator(16, L, src, points, metric=nb.DEMOD_MAXLOG)
    c = points[idx]
    rows = []
    for label, gain in channels:
        res = dict(channel=label, frames=B, code=NAME, cells=[])
        for ebn0 in ebn0s:
            sigma = float(np.sqrt(1.0 / (2.0 * m * (K / N) * 10.0 ** (ebn0 / 10.0))))   # unit-energy points, E|h|^2 = 1
            if gain is None:
                rx = c + sigma * noise
            else:
                rx = np.stack([gain[..., 0] * c[..., 0] - gain[..., 1] * c[..., 1], gain[..., 0] * c[..., 1] + gain[..., 1] * c[..., 0]], axis=-1) + sigma * noise
            dec.decode_samples_idd(rx, sigma, 3, gain=gain)                     # warm-up: buffers exist
            for passes in (1, 2, 3):
                t = time.perf_counter()
                out, conv, its, used = dec.decode_samples_idd(rx, sigma, passes, gain=gain)
                dt = time.perf_counter() - t
                cell = dict(ebn0=ebn0, sigma=sigma, passes=passes, frame_errors=int((out[:, :K] != msg).any(axis=1).sum()),
                            unconverged=int((conv == 0).sum()), iterations_per_frame=float((its + (used - 1) * MAX_ITER).mean()), frames_per_second=B / dt)
                res["cells"].append(cell)
                rows.append((label,) + tuple(cell[k] for k in ("ebn0", "passes", "frame_errors", "unconverged", "iterations_per_frame", "frames_per_second")))
        print(json.dumps(res), flush=True)
    dec.close()
    print("| channel | Eb/N0 | passes | frame errors of %d | unconverged | iterations / frame | frames / s |" % B)
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.2f | %d | %d | %d | %.2f | %.0f |" % r)


def demod_times(argv):
    B0 = int(argv[0]) if len(argv) > 0 else 0                                # 0: each case at its own batch
    repeats = int(argv[1]) if len(argv) > 1 else 5
    gf64 = nb.Code(NAME)
    c256 = nb.Code("divsalar.CNBLDPC.512.256.GF.256")
    u256 = nb.Code("divsalar.UNBLDPC.512.256.GF.256")
    # label, graph, order, constellation, src, L, decoder parameters, batch (configurations 4 and 5: tools/bench_config.py)
    cases = [("general: GF(64), 16-QAM interleaved", gf64, 16, CONS, np.random.default_rng(SEED).permutation(gf64.N * 6).astype(np.int32), gf64.N * 6 // 4, KW, 4096),
             ("q-ary: GF(64), 64-QAM (configuration 4)", gf64, 64, "GRAY_64QAM", np.arange(gf64.N, dtype=np.int32), gf64.N, KW, 8192),
             ("q-ary: GF(256), 256-QAM (configuration 5)", c256, 256, "GRAY_256QAM", np.arange(c256.N, dtype=np.int32), c256.N, dict(ems_nm=32, ems_nc=3), 1024),
             ("BPSK: GF(256), U512.256 (L = 512)", u256, 2, "BPSK", np.arange(u256.N * 8, dtype=np.int32), u256.N * 8, dict(ems_nm=32, ems_nc=3), 4096)]
    print("| demodulator | what | ms (median of %d) | min .. max |" % repeats)
    print("|---|---|---|---|")
    for label, code, M, cons, src, L, kw, batch in cases:
        B = B0 or batch
        state = np.random.default_rng(1).integers(1, 30000, (B, 3)).astype(np.uint32)
        points = np.array([[x[1], x[2]] for x in sorted(df.constellation(cons))], dtype=np.float64)
        dec = nb.Decoder(code, nb.METHOD_EMS, 2, poll_every=POLL, max_batch=B, device=0, **kw)
        if M == 16:
            dec.set_demodulator(M, L, src, points, metric=nb.DEMOD_MAXLOG)
        else:
            dec.set_demodulator(M, L, src, points)
        txi = np.zeros((B, L), dtype=np.uint8)
        res = dict(demodulator=label, batch=B)
        for fading in (False, True):
            dec.set_fading("rayleigh" if fading else None, 1)
            wall = []
            for k in range(repeats + 1):
                t = time.perf_counter()
                dec.channel_batch(0, txi, state, 0.5)
                if k:
                    wall.append((time.perf_counter() - t) * 1e3)
            key = "channel, rayleigh" if fading else "channel, awgn"
            res[key] = (statistics.median(wall), min(wall), max(wall))
            print("| %s | %s (wall) | %.3f | %.3f .. %.3f |" % ((label, key) + res[key]))
        for with_prior in ((False, True) if M == 16 else (False,)):
            for with_gain in (False, True):
                ms = [dec.time_demod(0, 0.5, B, with_prior, with_gain) for _ in range(repeats + 1)][1:]
                key = "demodulator%s%s" % (", prior" if with_prior else "", ", gains" if with_gain else "")
                res[key] = (statistics.median(ms), min(ms), max(ms))
                print("| %s | %s | %.4f | %.4f .. %.4f |" % ((label, key) + res[key]))
        dec.close()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["demod"]:
        demod_times(sys.argv[2:])
    else:
        fer_table(sys.argv[1:])
