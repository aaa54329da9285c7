#!/usr/bin/env python3
"""What iterative demapping buys in frame errors (numbers to record in DESIGN.md section 5i, not to assert).

BDS576.288 GF(64), EMS nm = 16 nc = 3, max_iter 50, early exit (poll_every 2), 16-QAM through a fixed random bit interleaver; 4096
random-message code words of the host chain (hostlib.frontend) per Eb/N0 point, modulated and sent through AWGN here (numpy, seeded),
decoded with passes = 1 / 2 / 3 (max-log demodulator, max-log extrinsic).  Run twice: with the shipped Gray table, and with the SAME
sixteen points in natural binary order (index = 4 * column + row) -- a permutation of the table made here, nothing shipped.  Per cell:
frame errors, iterations per frame (summed over the passes a frame ran), frames per second of the call (host wall clock, host buffers).

usage: python tools/idd_gain.py [frames] [EbN0 ...]     -- one JSON line per labelling, then a table; the default points cover both
waterfalls (Gray: 2.5 - 4.5 dB, natural order: 4 - 6 dB)"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
import nbldpc_amd.datafiles as df  # noqa: E402
from nbldpc_amd import hostlib  # noqa: E402
from nbldpc_amd.profiles import DEFAULTS  # noqa: E402

NAME, KW, MAX_ITER, POLL, CONS, SEED = "BDS.576.288.GF.64", dict(ems_nm=16, ems_nc=3), 50, 2, "GRAY_16QAM", 20260


def natural_order(points):
    """the same points, index = 4 * (rank of the real part) + (rank of the imaginary part)"""
    lv = np.sort(np.unique(np.round(points[:, 0], 12)))
    assert len(lv) == 4
    nat = np.array([[lv[c >> 2], lv[c & 3]] for c in range(16)])
    assert sorted(map(tuple, np.round(nat, 9))) == sorted(map(tuple, np.round(points, 9)))
    return nat


def modulate(tx, p, src, m, L):
    """constellation index of every point: label bit t = s m + i (weight 2^(m-1-i)) carries code bit g with src[g] == t"""
    bits = ((tx[:, :, None] >> np.arange(p)) & 1).reshape(tx.shape[0], -1)      # code bit g = n p + j
    label = np.zeros((tx.shape[0], L * m), dtype=np.int64)
    label[:, src] = bits
    return (label.reshape(tx.shape[0], L, m) << (m - 1 - np.arange(m))).sum(axis=2)


def main():
    argv = sys.argv[1:]
    B = int(argv[0]) if len(argv) > 0 else 4096
    ebn0s = [float(x) for x in argv[1:]] or [3.0, 3.5, 4.0, 4.5, 5.5, 6.0]   # Gray falls between 2.5 and 4.5 dB, natural order between 4 and 6
    code = nb.Code(NAME)
    N, q, K = code.N, code.q, code.N - code.M
    p = q.bit_length() - 1
    gray = np.array([[x[1], x[2]] for x in sorted(df.constellation(CONS))], dtype=np.float64)
    m = 4
    L = N * p // m
    src = np.random.default_rng(SEED).permutation(N * p).astype(np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        prof = {k: v for k, v in dict(DEFAULTS, gfq=q, method=2, max_iter=MAX_ITER, parallel=B, **KW).items() if k not in ("code", "constellation")}
        hostlib.prepare_workdir(tmp, dict(prof, code=NAME, random_msg=1), NAME, "BPSK")
        _, tx, msg, _ = hostlib.frontend(tmp, 5.0, 1, N, K, q, B)
    idx = modulate(tx, p, src, m, L)
    noise = np.random.default_rng(SEED + 1).standard_normal((B, L, 2))
    rows = []
    for label, points in (("gray", gray), ("natural", natural_order(gray))):
        dec = nb.Decoder(code, nb.METHOD_EMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **KW)
        dec.set_demodulator(16, L, src, points, metric=nb.DEMOD_MAXLOG)
        res = dict(labelling=label, frames=B, code=NAME, cells=[])
        for ebn0 in ebn0s:
            sigma = float(np.sqrt(1.0 / (2.0 * m * (K / N) * 10.0 ** (ebn0 / 10.0))))   # unit-energy points, m R information bits each
            rx = points[idx] + sigma * noise
            dec.decode_samples_idd(rx, sigma, 3)                                 # warm-up: buffers exist
            for passes in (1, 2, 3):
                t = time.perf_counter()
                out, conv, its, used = dec.decode_samples_idd(rx, sigma, passes)
                dt = time.perf_counter() - t
                ferr = int((out[:, :K] != msg).any(axis=1).sum())
                total_its = float((its + (used - 1) * MAX_ITER).mean())          # a frame that went on ran max_iter in every earlier pass
                cell = dict(ebn0=ebn0, sigma=sigma, passes=passes, frame_errors=ferr, unconverged=int((conv == 0).sum()),
                            iterations_per_frame=total_its, frames_per_second=B / dt)
                res["cells"].append(cell)
                rows.append((label,) + tuple(cell[k] for k in ("ebn0", "passes", "frame_errors", "unconverged", "iterations_per_frame", "frames_per_second")))
        dec.close()
        print(json.dumps(res), flush=True)
    print("| labelling | Eb/N0 | passes | frame errors of %d | unconverged | iterations / frame | frames / s |" % B)
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.2f | %d | %d | %d | %.2f | %.0f |" % r)


if __name__ == "__main__":
    main()
