#!/usr/bin/env python3
"""Generate the ordered-statistics decoding (OSD post-processing, decode method 6) fixtures from the COMPILED REFERENCE (oracle/_ref,
see oracle/Makefile `make ref`).

Build-container only, like make_golden.py, whose driver calls and packing it reuses by import:
  fer_anchors_osd.json  FER lines of the reference's main loop for OSD profiles (kept apart from fer_anchors.json, whose keys
                tests/test_gpu_fer.py parametrizes over)
  osd_*.npz     the arrays make_golden.py documents (outputs at several iteration counts, subsampled state); low iteration counts, so
                that most frames go through OSD.  osd_flag0_gf16 keeps the posteriors of frame 0 after every iteration 1..5, from
                which the flag-0 reliabilities are rebuilt.

usage: python tests/golden/make_golden_osd.py [set ... | fer:<set> ...]      (no argument: everything)
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
    # EMS, GF(16) 128.64 (128 bits), order 2, no CRC rows
    "osd_ems_gf16_o2": ("O2", dict(gfq=16, code=mg.U128_16, method=2, max_iter=5, parallel=4, ems_nm=8, ems_nc=2, osd_order=2, osd_flag=1,
                                   constellation="BPSK"), 1.0, 4, [1, 2, 5], [1], [0]),
    # T-EMS, GF(256) 128.64, order 1, eight CRC-8 rows
    "osd_tems_gf256_o1_crc8": ("O2", dict(gfq=256, code=mg.U128_256, method=4, max_iter=5, parallel=4, tems_nr=2, tems_nc=3, osd_order=1,
                                          osd_flag=1, crc_len=8, crc_correct=8, constellation="BPSK"), 1.5, 4, [1, 2, 5], [1], [0]),
    # BP (O0 build: the reference's BP falls off its end after OSD), GF(16), order 3, sixteen CRC-16 rows
    "osd_bp_gf16_o3_crc16": ("O0", dict(gfq=16, code=mg.U128_16, method=1, max_iter=5, parallel=2, osd_order=3, osd_flag=1, crc_len=16,
                                        crc_correct=16, constellation="BPSK"), 1.0, 3, [1, 2, 5], [1], [0]),
    # BS-TEMS, GF(16), order 2, 24 CRC-24 rows
    "osd_bstems_gf16_o2_crc24": ("O2", dict(gfq=16, code=mg.U128_16, method=7, max_iter=5, parallel=4, bs_nm=4, bs_nc=2, osd_order=2,
                                            osd_flag=1, crc_len=24, crc_correct=24, constellation="BPSK"), 1.0, 3, [1, 2, 5], [1], [0]),
    # method 6 alone: GF(64) BDS 576.288 over 64-QAM (all-zero codeword), order 1
    "osd_m6_bds_qam": ("O2", dict(gfq=64, code=mg.BDS, method=6, max_iter=5, parallel=2, osd_order=1, osd_flag=1, nqam=64,
                                  constellation="GRAY_64QAM", random_msg=0), 4.0, 2, [1], [], []),
    # T-EMS post-processing on the GF(64) BDS 576.288 code, BPSK, random codewords, order 1: the distance covers 575 of its 576 bits
    # (compute_min_distance_bit's truncated CodeLen_bit) and so does the copy of a winner, so the last bit keeps the base word's value
    # -- in about one frame of five at 1 dB the winner's last bit differs from it
    "osd_tems_bds_o1": ("O2", dict(gfq=64, code=mg.BDS, method=4, max_iter=2, parallel=4, tems_nr=2, tems_nc=3, osd_order=1, osd_flag=1,
                                   constellation="BPSK", random_msg=1), 1.0, 3, [1, 2], [], []),
    # method 6 alone: GF(256) 128.64, order 2
    "osd_m6_gf256_o2": ("O2", dict(gfq=256, code=mg.U128_256, method=6, max_iter=5, parallel=4, osd_order=2, osd_flag=1,
                                   constellation="BPSK"), 1.5, 4, [1], [], []),
    # flag 0 (posterior sums, factor 0.5), EMS GF(16), order 1; posteriors of frame 0 after 1..5 iterations
    "osd_flag0_gf16": ("O2", dict(gfq=16, code=mg.U128_16, method=2, max_iter=5, parallel=4, ems_nm=8, ems_nc=2, osd_order=1, osd_flag=0,
                                  osd_factor=0.5, constellation="BPSK"), 1.0, 4, [1, 2, 5], [1, 2, 3, 4, 5], [0]),
}

FER_SETS = {
    # EMS GF(16) 128.64, 5 iterations, OSD order 1 on every failed frame, 8 CRC-8 rows
    "osd_ems_gf16_o1_crc8_p8": ("O2", dict(gfq=16, code=mg.U128_16, method=2, max_iter=5, parallel=8, ems_nm=8, ems_nc=2, osd_order=1, osd_flag=1,
                                           crc_len=8, crc_correct=8, snr_begin=1.5, snr_step=0.5, snr_stop=2.5, constellation="BPSK",
                                           min_sim_cycle=400)),
    # method 6 alone, GF(256) 128.64, order 2
    "osd_m6_gf256_o2_p8": ("O2", dict(gfq=256, code=mg.U128_256, method=6, max_iter=5, parallel=8, osd_order=2, osd_flag=1,
                                      snr_begin=2.0, snr_step=1.0, snr_stop=3.0, constellation="BPSK", min_sim_cycle=200)),
    # T-EMS post-processing on the BDS code, BPSK, random codewords, order 1 (the truncated bit count, above)
    "osd_tems_bds_o1_p4": ("O2", dict(gfq=64, code=mg.BDS, method=4, max_iter=3, parallel=4, tems_nr=2, tems_nc=3, osd_order=1, osd_flag=1,
                                      constellation="BPSK", random_msg=1, snr_begin=1.0, snr_step=1.0, snr_stop=2.0, min_sim_cycle=120)),
    # flag 0 (factor 0.5), T-EMS GF(16) 128.64, order 2
    "osd_tems_gf16_flag0_p8": ("O2", dict(gfq=16, code=mg.U128_16, method=4, max_iter=5, parallel=8, tems_nr=2, tems_nc=2, osd_order=2,
                                          osd_flag=0, osd_factor=0.5, snr_begin=1.5, snr_step=1.0, snr_stop=2.5, constellation="BPSK",
                                          min_sim_cycle=200)),
}


def run_fer(names):
    path = os.path.join(mg.GOLD, "fer_anchors_osd.json")
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
            p["cpu_s_per_frame"] = p.pop("cpu_s", 0.0) / max(1, p["frames"])  # the reference's CPU time, for DESIGN.md
        anchors[name] = dict(profile=dict(kw), code=code, constellation=cons, points=pts)
        shutil.rmtree(tmp)
        print(f"fer {name}: {pts} ({time.time() - t0:.1f}s)")
    json.dump(anchors, open(path, "w"), indent=1)


def run_set(name):
    mg.SETS[name] = SETS[name]
    mg.run_set(name)


if __name__ == "__main__":
    args = sys.argv[1:] or list(SETS) + ["fer:" + k for k in FER_SETS]
    for a in args:
        if not a.startswith("fer:"):
            run_set(a)
    fer = [a[4:] for a in args if a.startswith("fer:")]
    if fer:
        run_fer(fer)
