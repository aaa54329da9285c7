#!/usr/bin/env python3
"""Generate the deg_wide_*_bp.npz fixtures: the COMPILED REFERENCE (oracle/_ref, see oracle/Makefile `make ref`; absent from a fresh
checkout, build it first) running method 1, exact log-domain QSPA, on synthetic graphs of tests/degree_util.py whose checks have degree
9 .. 32 (GF(256): 5, 8, 9, 16) -- above everything make_golden_degrees.py covers for method 1.  The reference's Decoding_BP sizes its
arrays by the maxChkDegree of the code file, so it runs these graphs as they are.

The driver is the one whose NBLDPC.cpp is compiled at -O0, as for every method-1 set of make_golden_degrees.py: Decoding_BP ends without a
return statement when a frame does not converge, which an optimising build is free to miscompile (it does: the -O2 driver aborts).

Build-container only, and modelled on make_golden_tems_wide.py: the graph is written as a reference-format code file and decoded by
`ref_driver decode` on channel LLRs made here -- all-zero-codeword BPSK / AWGN LLRs at the graph's own rate 1 - M/N, real-valued.
CNBLDPC::Initial needs N > M and a bit-level H of full row rank; a seed whose graph it cannot initialise within the time limit is passed
over.
Each file holds L_ch [F][N][q-1], out / ret / syn_ok [K][F] at iters[k], st_post / st_v2c / st_c2v after state_iters[k] iterations
for the frames in state_lanes, and in `meta` the profile and the graph (`spec`).

Cost of the reference.  It re-derives the forward and backward partials for every output edge (NBLDPC.cpp:751-754) and evaluates every
term of every log-sum-exp with expl / logl in 80-bit arithmetic: about dc (dc - 2) q^2 such terms per check and iteration, 3.9 million
for one degree-32 check over GF(64) and 14.7 million for one degree-16 check over GF(256).  Frames and iteration counts are sized to
that: the time limit stays 60 s.
Size.  Every file stays below the largest deg_* fixture (deg_dc78_gf64_ems, 487 kB): the graphs have 6 checks (GF(256): 4, the
degree-2-variable graph of the T-EMS fixture), the state is that of frame 0.

usage: python tests/golden/make_golden_bp_wide.py [set ...]      (no argument: everything)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
import degree_util as du  # noqa: E402
from make_golden_degrees import GOLD, REF, RUN  # noqa: E402
from make_golden_ems_wide import frames  # noqa: E402
from make_golden_tems_wide import MAX_BYTES, TIME_LIMIT, WIDE  # noqa: E402
from nbldpc_amd.profiles import profile_text  # noqa: E402

# name -> ((check degrees, variable degrees, M), q, profile kwargs, iters, state_iters, Eb/N0 of every frame in dB)
SETS = {
    "deg_wide_gf64_bp": ((WIDE, (2, 3), 6), 64, dict(method=1), [1, 2, 5], [1, 2], (3, 5, 6, 8)),
    "deg_wide_gf16_bp": ((WIDE, (2, 3), 6), 16, dict(method=1), [1, 2, 5, 12], [1, 2], (3, 4, 5, 5, 6, 6, 7, 8)),
    # (the (5, 8, 9, 16) graph of deg_wide_gf256_tems: 38 sockets, all variables of degree 2, N = 19)
    "deg_wide_gf256_bp": (((5, 8, 9, 16), (2,), 4), 256, dict(method=1), [1, 2, 4], [1], (3, 6)),
}


def run_set(name):
    prof, q, kw, iters, st_iters, levels = SETS[name]
    for seed in range(9100, 9140):
        code, _, spec = du.degree_code(q, seed, prof[0], prof[1], prof[2])
        if code.N <= code.M:
            continue
        L = frames(code, seed, levels)
        tmp = tempfile.mkdtemp(prefix="golden_")
        du.write_spec_code_file(spec, os.path.join(tmp, "code.txt"))
        L.tofile(os.path.join(tmp, "L_ch.bin"))
        pk = dict(kw, gfq=q, code=os.path.join(tmp, "code.txt"), max_iter=max(iters), parallel=1, crc_len=8, random_msg=0,
                  constellation=REF + "BPSK.txt")
        prof_path = os.path.join(tmp, "profile.txt")
        open(prof_path, "w").write(profile_text(**pk))
        t0 = time.time()
        try:
            subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "ref_driver_O0"), "decode", prof_path, tmp,
                                   os.path.join(tmp, "L_ch.bin"), str(L.shape[0]), ",".join(map(str, iters)), ",".join(map(str, st_iters)), "1"],
                                  cwd=RUN, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL, timeout=TIME_LIMIT)
        except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as e:
            print(f"{name}: seed {seed}: the reference did not finish ({type(e).__name__}); next seed")
            shutil.rmtree(tmp)
            continue
        break
    else:
        raise SystemExit(f"{name}: no graph the reference initialises")
    dt = time.time() - t0
    arrs = {k[:-4]: np.load(os.path.join(tmp, k)) for k in os.listdir(tmp) if k.endswith(".npy")}
    arrs["L_ch"] = L
    arrs["state_lanes"] = np.array([0], dtype=np.int32)
    meta = dict(profile=dict(kw, gfq=q, max_iter=max(iters)), spec=spec, seed=seed, build="O0", ebn0_db=list(levels),
                chk_degs=sorted(set(code.chk_deg.tolist())), var_degs=sorted(set(code.var_deg.tolist())),
                reference_flags="-std=c++14 -O2 (NBLDPC.cpp at -O0) -ffp-contract=off, g++ 11.4, x86-64")
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrs)
    shutil.rmtree(tmp)
    size = os.path.getsize(path)
    print(f"{name}: seed {seed} N={code.N} E={code.E} ret={arrs['ret'].tolist()} syn_ok={arrs['syn_ok'].tolist()} "
          f"(reference {dt:.1f}s, {size / 1e3:.0f} kB)")
    assert size < MAX_BYTES, (size, MAX_BYTES)
    assert {k: arrs[k].shape[1] for k in ("st_post", "st_v2c", "st_c2v")} == dict(st_post=1, st_v2c=1, st_c2v=1)


if __name__ == "__main__":
    for n in sys.argv[1:] or list(SETS):
        run_set(n)
