#!/usr/bin/env python3
"""Generate the basic-set T-EMS (decode method 7) fixtures from the COMPILED REFERENCE (oracle/_ref, see oracle/Makefile `make ref`).

Build-container only, like make_golden.py, whose driver calls and packing it reuses by import:
  bstems_*.npz                 the arrays make_golden.py documents (outputs at several iteration counts, subsampled state)
  fer_anchors_bstems.json      FER lines of the reference's main loop for method-7 profiles (kept apart from fer_anchors.json,
                               whose keys tests/test_gpu_fer.py parametrizes over)

usage: python tests/golden/make_golden_bstems.py [set ... | fer:<set> ...]      (no argument: everything)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from nbldpc_amd.profiles import profile_text  # noqa: E402

# name -> (driver build, profile kwargs, EbN0, frames, iters, state_iters, state_lanes), as make_golden.SETS
SETS = {
    # nm = p = 4 (greedy basis of the whole field), nc = 2
    "bstems_gf16_u128": ("O2", dict(gfq=16, code=mg.U128_16, method=7, max_iter=20, parallel=4, bs_nm=4, bs_nc=2,
                                    constellation="BPSK"), 2.0, 4, [1, 2, 5, 20], [1, 2, 3], [0, 1]),
    # check degrees 4 / 5 mixed, nm = 6 > p (the six smallest symbols), factor / offset
    "bstems_gf16_u512_mixed": ("O2", dict(gfq=16, code=mg.U512_16, method=7, max_iter=20, parallel=4, bs_nm=6, bs_nc=3,
                                          bs_factor=1.1, bs_offset=0.05, constellation="BPSK"), 2.0, 4, [1, 2, 5, 20], [1, 2], [0, 1]),
    # GF(64) BDS, 64-QAM, all-zero codeword; the waterfall of nm = 6 sits above 4 dB
    "bstems_bds_qam": ("O2", dict(gfq=64, code=mg.BDS, method=7, max_iter=50, parallel=2, bs_nm=6, bs_nc=3, nqam=64,
                                  constellation="GRAY_64QAM", random_msg=0), 4.5, 3, [1, 2, 5, 50], [1, 2], [0]),
    # GF(256): nm = p = 8, nc = 3
    "bstems_gf256_u128": ("O2", dict(gfq=256, code=mg.U128_256, method=7, max_iter=50, parallel=4, bs_nm=8, bs_nc=3,
                                     constellation="BPSK"), 2.5, 4, [1, 2, 5, 50], [1, 2], [0]),
    # GF(256): nm = 5 < p (the first five vectors of the greedy basis)
    "bstems_gf256_nm5": ("O2", dict(gfq=256, code=mg.U256_256, method=7, max_iter=30, parallel=3, bs_nm=5, bs_nc=2,
                                    constellation="BPSK"), 2.5, 2, [1, 2, 5, 30], [1, 2], [0]),
    # GF(256): nm = 12 > p, nc = 2
    "bstems_gf256_nm12": ("O2", dict(gfq=256, code=mg.U256_256, method=7, max_iter=30, parallel=3, bs_nm=12, bs_nc=2,
                                     constellation="BPSK"), 2.5, 2, [1, 2, 5, 30], [1, 2], [0]),
}

FER_SETS = {
    # GF(16) 512.256 (check degrees 4 / 5), nm = p = 4, nc = 2: 2000 frames per point through the waterfall
    "bstems_gf16_u512_p8": ("O2", dict(gfq=16, code=mg.U512_16, method=7, max_iter=20, parallel=8, bs_nm=4, bs_nc=2,
                                       snr_begin=1.5, snr_step=0.5, snr_stop=2.5, constellation="BPSK", min_sim_cycle=2000)),
    # GF(256) 128.64, nm = 8, nc = 3
    "bstems_gf256_u128_p8": ("O2", dict(gfq=256, code=mg.U128_256, method=7, max_iter=50, parallel=8, bs_nm=8, bs_nc=3,
                                        snr_begin=2.0, snr_step=1.0, snr_stop=3.0, constellation="BPSK", min_sim_cycle=400)),
    # GF(64) BDS, 64-QAM, all-zero codeword, nm = 6, nc = 3
    "bstems_bds_p4": ("O2", dict(gfq=64, code=mg.BDS, method=7, max_iter=50, parallel=4, bs_nm=6, bs_nc=3, nqam=64,
                                 constellation="GRAY_64QAM", random_msg=0, snr_begin=5.0, snr_step=1.0, snr_stop=6.0, min_sim_cycle=200)),
}


def run_set(name):
    mg.SETS[name] = SETS[name]
    mg.run_set(name)


def run_fer(names):
    path = os.path.join(mg.GOLD, "fer_anchors_bstems.json")
    anchors = json.load(open(path)) if os.path.exists(path) else {}
    for name in names:
        build, kw = FER_SETS[name]
        pk, code, cons = mg.resolve(kw)
        tmp = tempfile.mkdtemp(prefix="golden_")
        prof = os.path.join(tmp, "profile.txt")
        open(prof, "w").write(profile_text(**pk))
        t0 = time.time()
        out = subprocess.run([os.path.join(mg.ROOT, "oracle", "_ref", f"ref_driver_{build}"), "fer", prof], cwd=mg.RUN,
                             capture_output=True, text=True, check=True).stdout
        pts = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
        for p in pts:
            p.pop("cpu_s", None)
        anchors[name] = dict(profile=dict(kw), code=code, constellation=cons, points=pts)
        shutil.rmtree(tmp)
        print(f"fer {name}: {pts} ({time.time() - t0:.1f}s)")
    json.dump(anchors, open(path, "w"), indent=1)


if __name__ == "__main__":
    args = sys.argv[1:] or list(SETS) + ["fer:" + k for k in FER_SETS]
    fer = [a[4:] for a in args if a.startswith("fer:")]
    for a in args:
        if not a.startswith("fer:"):
            run_set(a)
    if fer:
        run_fer(fer)
