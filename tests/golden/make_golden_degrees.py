#!/usr/bin/env python3
"""Generate the deg_*.npz fixtures: the COMPILED REFERENCE (oracle/_ref, see oracle/Makefile `make ref`) on the synthetic graphs of
tests/degree_util.py, whose check degrees (2 .. 8) and variable degrees (1 .. 8) no shipped code has.

Build-container only, like make_golden.py.  The graph of a set is written as a reference-format code file
(degree_util.write_spec_code_file) and decoded by `ref_driver decode`: CNBLDPC::Initial + CNBLDPC::Decoding on channel LLRs made
here (tiny irregular graphs have no code rate worth a link chain) -- all-zero-codeword BPSK / AWGN LLRs at five noise levels.
Real-valued and free of ties on purpose: the canonical restatements and the kernels are held to the reference on every frame,
and where exact ties meet inexact sums the reference's running add-then-subtract residue decides; ties
and erasures run against the restatements in tests/test_gpu_degrees.py.
Each file holds L_ch [8][N][q-1], out / ret / syn_ok [K][8] at iters[k], st_post / st_v2c / st_c2v after state_iters[k]
iterations for frames 0 and 1, and in `meta` the profile and the graph (`spec`), so the tests rebuild nothing.

Time of the reference per set on one core, g++ -O2 (log-QSPA: -O0), measured: 0.0 - 0.6 s, deg_dc78_gf64_ems 1.5 s -- its
recursion prunes at nc deviations, so (nm 6-8, nc 2) and (nr 2, nc 3) stay cheap at check degree 8.

usage: python tests/golden/make_golden_degrees.py [set ...]      (no argument: everything)
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import degree_util as du  # noqa: E402
from nbldpc_amd.profiles import profile_text  # noqa: E402

REF = "/root/reference/"
RUN = os.path.join(ROOT, "oracle", "_ref", "run")
GOLD = os.path.join(ROOT, "tests", "golden")

# The reference's CNBLDPC::Initial also builds its OSD and CRC matrices: it needs more variables than checks ((N - M) log2(q) bits
# above crcLen, which must be 8, 16 or 24) and a bit-level H of full row rank, or its eliminations never end.  The grid graphs of
# degree_util.profile_code are not made for that (dv48 has N < M, `all` has N - M = 2), so the sets below keep each profile's degree
# SETS but weight the small variable degrees, and dv48 -- variables of degree 4 .. 8 -- takes checks of degree 7 / 8, the only way
# to more variables than checks.  A seed whose graph the reference cannot initialise within 20 s is passed over.
LOW = (1, 2, 3, 4, 1, 2, 3, 5, 1, 2, 3, 6, 2, 2, 3, 7, 2, 2, 3, 8)
ALL_CHK = (2, 3, 4, 5, 6, 7, 8)
# name -> (driver build, (check degrees, variable degree cycle, M), q, profile kwargs, iters, state_iters)
SETS = {
    "deg_all_gf16_ems": ("O2", (ALL_CHK, LOW, 14), 16, dict(method=2, ems_nm=6, ems_nc=2, ems_factor=1.1, ems_offset=0.1), [1, 2, 5, 12], [1, 2]),
    "deg_all_gf16_tems": ("O2", (ALL_CHK, LOW, 14), 16, dict(method=4, tems_nr=2, tems_nc=3, tems_factor=1.1, tems_offset=0.05), [1, 2, 5, 12], [1, 2]),
    "deg_all_gf16_bp": ("O0", (ALL_CHK, LOW, 14), 16, dict(method=1), [1, 2, 3], [1, 2]),
    "deg_all_gf16_bstems": ("O2", (ALL_CHK, LOW, 14), 16, dict(method=7, bs_nm=6, bs_nc=2), [1, 2, 5, 12], [1, 2]),
    "deg_dc78_gf64_ems": ("O2", ((7, 8), (2, 3), 12), 64, dict(method=2, ems_nm=8, ems_nc=2), [1, 2, 5, 12], [1, 2]),
    "deg_dv48_gf4_tems": ("O2", ((7, 8), (4, 5, 6, 7, 8), 24), 4, dict(method=4, tems_nr=2, tems_nc=3), [1, 2, 5, 12], [1, 2]),
    "deg_dc2_gf256_bp": ("O0", ((2,), (1, 2), 12), 256, dict(method=1), [1, 2, 3], [1]),
}


def frames(code, seed):
    """8 frames: all-zero-codeword BPSK LLRs (rate-1/2 convention) at 5 noise levels."""
    rng = np.random.default_rng(seed)
    p = code.q.bit_length() - 1
    a = np.arange(1, code.q)
    mask = ((a[:, None] >> np.arange(p)[None, :]) & 1).astype(np.float64)
    L = []
    for ebn0 in (0.0, 0.0, 2.0, 2.0, 4.0, 4.0, 1.0, 3.0):
        sigma = 1.0 / np.sqrt(2 * 0.5 * 10 ** (ebn0 / 10.0))
        bit = -2.0 * (1.0 + sigma * rng.standard_normal((code.N, p))) / sigma ** 2
        L.append(bit @ mask.T)
    return np.array(L)


def run_set(name):
    build, prof, q, kw, iters, st_iters = SETS[name]
    for seed in range(9000, 9040):
        code, _, spec = du.degree_code(q, seed, prof[0], prof[1], prof[2])
        L = frames(code, seed)
        tmp = tempfile.mkdtemp(prefix="golden_")
        du.write_spec_code_file(spec, os.path.join(tmp, "code.txt"))
        L.tofile(os.path.join(tmp, "L_ch.bin"))
        pk = dict(kw, gfq=q, code=os.path.join(tmp, "code.txt"), max_iter=max(iters), parallel=1, crc_len=8, random_msg=0,
                  constellation=REF + "BPSK.txt")
        prof_path = os.path.join(tmp, "profile.txt")
        open(prof_path, "w").write(profile_text(**pk))
        t0 = time.time()
        try:
            subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", f"ref_driver_{build}"), "decode", prof_path, tmp,
                                   os.path.join(tmp, "L_ch.bin"), str(L.shape[0]), ",".join(map(str, iters)), ",".join(map(str, st_iters)), "2"],
                                  cwd=RUN, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL, timeout=20)
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
    arrs["state_lanes"] = np.array([0, 1], dtype=np.int32)
    meta = dict(profile=dict(kw, gfq=q, max_iter=max(iters)), spec=spec, seed=seed, build=build,
                chk_degs=sorted(set(code.chk_deg.tolist())), var_degs=sorted(set(code.var_deg.tolist())),
                reference_flags="-std=c++14 -O2 (NBLDPC.cpp at -%s) -ffp-contract=off, g++ 11.4, x86-64" % build)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrs)
    shutil.rmtree(tmp)
    print(f"{name}: seed {seed} N={code.N} E={code.E} ret={arrs['ret'].tolist()} syn_ok={arrs['syn_ok'].tolist()} "
          f"(reference {dt:.1f}s, {os.path.getsize(path) / 1e3:.0f} kB)")


if __name__ == "__main__":
    for n in sys.argv[1:] or list(SETS):
        run_set(n)
