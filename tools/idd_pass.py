#!/usr/bin/env python3
"""What iterative demapping costs beside the calls it is built from (numbers to record in DESIGN.md section 5i, not to assert).

BDS576.288 GF(64), EMS nm = 16 nc = 3, max_iter 50, early exit with the harness's poll_every (2), Gray 16-QAM through a fixed random
bit interleaver, batch 4096; the all-zero word through the device channel, samples resident in a slot.  One warm-up, median of
`repeats` (5) with its range:

  demodulator, no prior / with a prior    ONE launch of demod_general_kernel<false> / <true> between two events on the decoder's
                                          stream (nbl_debug_time_demod)
  soft output, a-posteriori / extrinsic   nbl_soft_output_device / _ex, bit LLRs only, events on the caller's stream, after a decode
  plain call, then again at the end       nbl_decode_batch_resident, host wall clock: two sets of the same call show the spread
  passes = 1 / 2 / 3                      nbl_decode_batch_resident_idd, host wall clock of the call (it synchronises itself), at the
                                          sigma where about `fail` (10 %) of the frames fail pass 1 (found by bisection on pass 1);
                                          the survivor count per pass is that of passes = 3

usage: python tools/idd_pass.py [batch] [repeats] [fail]     -- one JSON line, then a table"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
import nbldpc_amd.datafiles as df  # noqa: E402

NAME, KW, MAX_ITER, POLL, CONS, SEED = "BDS.576.288.GF.64", dict(ems_nm=16, ems_nc=3), 50, 2, "GRAY_16QAM", 20260


def interleaved_src(N, p, m):
    """a fixed random bit interleaver: code bit g on label bit src[g], every label bit claimed"""
    assert (N * p) % m == 0
    return np.random.default_rng(SEED).permutation(N * p).astype(np.int32), N * p // m


def median3(ms):
    return statistics.median(ms), min(ms), max(ms)


def timed_events(fn, repeats):
    ms = []
    for k in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k:
            ms.append(a.elapsed_time(b))
    return median3(ms)


def timed_wall(fn, repeats):
    ms = []
    for k in range(repeats + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if k:
            ms.append((time.perf_counter() - t) * 1e3)
    return median3(ms)


def main():
    argv = sys.argv[1:]
    B = int(argv[0]) if len(argv) > 0 else 4096
    repeats = int(argv[1]) if len(argv) > 1 else 5
    fail = float(argv[2]) if len(argv) > 2 else 0.10
    code = nb.Code(NAME)
    N, q = code.N, code.q
    p = q.bit_length() - 1
    points = np.array([[x[1], x[2]] for x in sorted(df.constellation(CONS))], dtype=np.float64)
    M = len(points)
    m = M.bit_length() - 1
    src, L = interleaved_src(N, p, m)
    dec = nb.Decoder(code, nb.METHOD_EMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **KW)
    dec.set_demodulator(M, L, src, points, metric=nb.DEMOD_MAXLOG)
    dec._tx_L = L
    state = np.random.default_rng(1).integers(1, 30000, (B, 3)).astype(np.uint32)
    txi = np.zeros((B, L), dtype=np.uint8)

    def failing(sigma):
        dec.channel_batch(0, txi, state, sigma)
        _, conv, _ = dec.decode_resident(0, sigma, B)
        return 1.0 - float(conv.mean())
    lo, hi = 0.2, 0.8                                   # failure rate rises with sigma
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        if failing(mid) < fail:
            lo = mid
        else:
            hi = mid
    sigma = 0.5 * (lo + hi)
    res = dict(batch=B, repeats=repeats, code=NAME, constellation=CONS, sigma=sigma, pass1_failure=failing(sigma))

    lib = dec.lib
    lib.nbl_debug_time_demod.restype = C.c_int
    lib.nbl_debug_time_demod.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_double)]

    def demod_ms(with_prior):
        out = []
        for k in range(repeats + 1):
            ms = C.c_double(0)
            dec._chk(lib.nbl_debug_time_demod(dec.h, 0, sigma, B, with_prior, C.byref(ms)))
            if k:
                out.append(ms.value)
        return median3(out)
    res["demod_no_prior_ms"] = demod_ms(0)
    res["demod_prior_ms"] = demod_ms(1)

    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    bits = torch.zeros((B, N * p), dtype=torch.float64, device="cuda")
    for key, soft in (("maxlog", "maxlog"), ("logsum", "logsum")):
        dec.decode_resident(0, sigma, B)
        res[f"soft_bits_{key}_ms"] = timed_events(lambda: dec.soft_output_device(soft, None, bits.data_ptr(), st), repeats)
        res[f"soft_bits_{key}_extrinsic_ms"] = timed_events(lambda: dec.soft_output_device(soft, None, bits.data_ptr(), st, extrinsic=True), repeats)

    def resident_idd(k):
        """nbl_decode_batch_resident_idd itself, also for passes = 1 (Decoder.decode_resident sends passes = 1 to the plain call)"""
        out = np.zeros((B, N), dtype=np.int32)
        conv, its, used = np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        idd = nb.binding.IddParams(k, nb.SOFT_MAXLOG)
        dec._chk(lib.nbl_decode_batch_resident_idd(dec.h, 0, sigma, B, C.byref(idd), out.ctypes.data, conv.ctypes.data, its.ctypes.data, used.ctypes.data))
        return out, conv, its, used

    res["plain_call_ms"] = timed_wall(lambda: dec.decode_resident(0, sigma, B), repeats)
    for k in (1, 2, 3):
        got = []
        res[f"passes_{k}_ms"] = timed_wall(lambda: got.append(resident_idd(k)), repeats)
        conv = got[-1][1]
        res[f"passes_{k}_unconverged"] = int((conv == 0).sum())
        res[f"passes_{k}_iterations_per_frame"] = float(got[-1][2].mean())
        if k == 3:
            used = got[-1][3]
            res["frames_entering_pass"] = [int((used >= j).sum()) for j in (1, 2, 3)]
    res["plain_call_again_ms"] = timed_wall(lambda: dec.decode_resident(0, sigma, B), repeats)   # the spread between two sets of the same call
    dec.close()
    print(json.dumps(res), flush=True)
    print("| what | ms (median of %d) | min .. max |" % repeats)
    print("|---|---|---|")
    for key in ("demod_no_prior_ms", "demod_prior_ms", "soft_bits_maxlog_ms", "soft_bits_maxlog_extrinsic_ms", "soft_bits_logsum_ms",
                "soft_bits_logsum_extrinsic_ms", "plain_call_ms", "passes_1_ms", "passes_2_ms", "passes_3_ms", "plain_call_again_ms"):
        print("| %s | %.3f | %.3f .. %.3f |" % ((key[:-3].replace("_", " "),) + tuple(res[key])))
    print("sigma %.4f, pass-1 failure %.3f; frames entering pass 1 / 2 / 3: %s; unconverged after 1 / 2 / 3 passes: %d / %d / %d"
          % (sigma, res["pass1_failure"], res["frames_entering_pass"], res["passes_1_unconverged"], res["passes_2_unconverged"],
             res["passes_3_unconverged"]))


if __name__ == "__main__":
    main()
