#!/usr/bin/env python3
"""What bit-LLR input and the soft-output pass cost beside the decode they wrap (numbers to record in DESIGN.md section 5h, not to assert).

Config 3's code and parameters: U512.256 GF(256), EMS nm = 32 nc = 3, max_iter 50, early exit with the harness's poll_every (2), batch
4096, the host link chain's random-message frames over BPSK / AWGN (hostlib.frontend), resident in HBM.  HIP events on the caller's
stream around each call, one warm-up, median of `repeats` (5):

  decode            nbl_decode_batch_device on the expanded L_ch; ms per iteration = call time / iterations launched
  decode_bits       nbl_decode_batch_bits_device on the per-bit LLRs of the same frames (same results)
  input, symbols    a max_iter = 0 decoder's nbl_decode_batch_device: init (the [q-1] -> [q] copy of L_ch) + output copies
  input, bits       the same decoder's nbl_decode_batch_bits_device: bits_to_lch_kernel + init + output copies
  soft, max-log     nbl_soft_output_device, sym_llr and bit_llr, after the decode
  soft, log-sum     the same with NBL_SOFT_LOGSUM
  soft, sym only / bits only (max-log)   which of the stores and the reductions the pass spends its time on

usage: python tools/soft_pass.py [batch] [repeats] [EbN0]     -- one JSON line, then a table"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import nbldpc_amd as nb  # noqa: E402
from nbldpc_amd import hostlib  # noqa: E402
from nbldpc_amd.profiles import DEFAULTS  # noqa: E402

NAME, KW, MAX_ITER, POLL = "divsalar.UNBLDPC.512.256.GF.256", dict(ems_nm=32, ems_nc=3), 50, 2


def timed(fn, repeats):
    """median milliseconds of fn() between two events on the current stream, after one warm-up call"""
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
    return statistics.median(ms), min(ms), max(ms)


def main():
    argv = sys.argv[1:]
    B = int(argv[0]) if len(argv) > 0 else 4096
    repeats = int(argv[1]) if len(argv) > 1 else 5
    ebn0 = float(argv[2]) if len(argv) > 2 else 1.5
    dev = torch.device("cuda", 0)
    code = nb.Code(NAME)
    N, q = code.N, code.q
    p = q.bit_length() - 1
    with tempfile.TemporaryDirectory() as tmp:
        prof = {k: v for k, v in dict(DEFAULTS, gfq=q, method=2, max_iter=MAX_ITER, parallel=B, **KW).items() if k not in ("code", "constellation")}
        hostlib.prepare_workdir(tmp, dict(prof, code=NAME), NAME, "BPSK")
        L, _, _, sigma = hostlib.frontend(tmp, ebn0, 1, N, N - code.M, q, B)
        rx, _, _, _ = hostlib.channel(tmp, ebn0, 1, N * p, B)
    lam = -2 * rx[:, :, 0] / (sigma * sigma)
    dL = torch.from_numpy(L).to(dev).contiguous()
    dlam = torch.from_numpy(np.ascontiguousarray(lam)).to(dev)
    del L, rx
    out = torch.zeros((B, N), dtype=torch.int32, device=dev)
    out2 = torch.zeros_like(out)
    conv = torch.zeros(B, dtype=torch.uint8, device=dev)
    its = torch.zeros(B, dtype=torch.int32, device=dev)
    sym = torch.zeros((B, N, q - 1), dtype=torch.float64, device=dev)
    bits = torch.zeros((B, N * p), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream()          # (a stream of the caller's: the NULL stream would mean "the decoder's own", which the events do not see)
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    assert st != 0
    res = dict(batch=B, ebn0=ebn0, repeats=repeats, code=NAME)

    dec = nb.Decoder(code, nb.METHOD_EMS, MAX_ITER, poll_every=POLL, max_batch=B, device=0, **KW)
    res["decode_ms"] = timed(lambda: dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), st), repeats)
    _, launches = dec.last_timing()
    res["iterations_launched"] = int(launches[1])
    res["ms_per_iteration"] = res["decode_ms"][0] / max(int(launches[1]), 1)
    res["decode_bits_ms"] = timed(lambda: dec.decode_bits_device(dlam.data_ptr(), B, out2.data_ptr(), conv.data_ptr(), its.data_ptr(), st), repeats)
    torch.cuda.synchronize()
    res["same_decisions"] = bool((out == out2).all().item())
    res["converged"] = int(conv.sum().item())
    for key, metric, s, b in (("soft_maxlog_ms", "maxlog", sym, bits), ("soft_logsum_ms", "logsum", sym, bits),
                              ("soft_sym_only_ms", "maxlog", sym, None), ("soft_bits_only_maxlog_ms", "maxlog", None, bits),
                              ("soft_bits_only_logsum_ms", "logsum", None, bits)):
        res[key] = timed(lambda: dec.soft_output_device(metric, s.data_ptr() if s is not None else None,
                                                        b.data_ptr() if b is not None else None, st), repeats)
    dec.close()
    dec0 = nb.Decoder(code, nb.METHOD_EMS, 0, poll_every=0, max_batch=B, device=0, **KW)
    res["input_symbols_ms"] = timed(lambda: dec0.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), st), repeats)
    res["input_bits_ms"] = timed(lambda: dec0.decode_bits_device(dlam.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), st), repeats)
    dec0.close()
    print(json.dumps(res), flush=True)
    print("| what | ms (median of %d) | min .. max |" % repeats)
    print("|---|---|---|")
    print("| one iteration of the decode (%d launched) | %.3f | |" % (res["iterations_launched"], res["ms_per_iteration"]))
    for key in ("decode_ms", "decode_bits_ms", "input_symbols_ms", "input_bits_ms", "soft_maxlog_ms", "soft_logsum_ms", "soft_sym_only_ms",
                "soft_bits_only_maxlog_ms", "soft_bits_only_logsum_ms"):
        print("| %s | %.3f | %.3f .. %.3f |" % ((key[:-3].replace("_", " "),) + tuple(res[key])))


if __name__ == "__main__":
    main()
