#!/usr/bin/env python3
"""Generate the field_*.npz fixtures: the COMPILED REFERENCE (oracle/_ref, see oracle/Makefile `make ref`)
run from a working directory whose SRC/Arith.Table.GF.<q>.txt and SRC/Mat.Repr.GF.<q>.txt were written by
nbldpc_amd/datafiles.py::write_gf_tables with a primitive polynomial OTHER than the one its shipped table files were made from.

Build-container only, like make_golden_degrees.py, whose frames (all-zero-codeword BPSK LLRs at five noise levels, real-valued and
free of ties) and file layout this follows: L_ch [8][N][q-1], out / ret / syn_ok [K][8] at iters[k], st_post / st_v2c / st_c2v after
state_iters[k] iterations for frames 0 and 1 (the GF(256) set: frame 0, to stay below the size of deg_dc2_gf256_bp), and in `meta` the profile, the graph (`spec`) and the modulus (`poly`).  The graphs:
the (2,4)-regular ring code of tests/field_util.py (fused specialised kernels) and the degree profile with every check degree
(general kernels); a seed whose graph the reference cannot initialise within 20 s is passed over, as there.

The GF(256) set needs a time limit of its own.  The reference's log-QSPA check node (NBLDPC.cpp: L_Back / L_Forward / LLR_BoxPlus)
recomputes the forward and backward recursions for every edge of a check, each step a q x q box-plus in exp / log arithmetic, and
log-QSPA runs on the -O0 driver: on the degree-4 checks of the ring code over GF(256) eight frames of three iterations take about
40 s -- with the default modulus as well, so it has nothing to do with the tables -- where deg_dc2_gf256_bp (checks of degree 2: no
recursion) takes under a second.

Only primitive moduli: the reference's loader reads q - 2 matrices from Mat.Repr, indexed by the powers of x, and a modulus that is
irreducible but not primitive has no such list.  Those moduli rest on the restatements alone (tests/field_util.py).

fer_anchors_fields.json holds one FER row of `ref_driver fer` (the reference's own main loop) for the harness test of
tests/test_gpu_fields.py: the GF(16) link shape of tests/link_shapes.py whose modulus is 25, EMS, 64 frames at 2 dB, run from a
work directory whose SRC/ holds the tables of that modulus; the row has error frames and error-free frames (asserted here).

usage: python tests/golden/make_golden_fields.py [set ... | fer]      (no argument: everything)
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
import field_util as fu  # noqa: E402
import nbldpc_amd.datafiles as df  # noqa: E402
from make_golden_degrees import ALL_CHK, LOW, REF, frames  # noqa: E402
from nbldpc_amd.profiles import profile_text  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")

# name -> (driver build, graph, q, modulus, profile kwargs, iters, state_iters[, time limit of the reference in seconds, state lanes]);
# graph: "ring" or (check degrees, variable degrees, M)
SETS = {
    "field_gf16_m25_ems": ("O2", (ALL_CHK, LOW, 14), 16, 25, dict(method=2, ems_nm=6, ems_nc=2, ems_factor=1.1, ems_offset=0.1), [1, 2, 5, 12], [1, 2]),
    "field_gf64_m91_tems": ("O2", "ring", 64, 91, dict(method=4, tems_nr=2, tems_nc=3, tems_factor=1.1, tems_offset=0.05), [1, 2, 5, 12], [1, 2]),
    "field_gf16_m25_bstems": ("O2", (ALL_CHK, LOW, 14), 16, 25, dict(method=7, bs_nm=6, bs_nc=2), [1, 2, 5, 12], [1, 2]),
    "field_gf256_m501_bp": ("O0", "ring", 256, 501, dict(method=1), [1, 2, 3], [1], 600, 1),
}

def run_set(name):
    build, graph, q, poly, kw, iters, st_iters = SETS[name][:7]
    limit, lanes = SETS[name][7:] if len(SETS[name]) > 7 else (20, 2)
    assert df.is_primitive(q, poly) and poly != df.PRIMITIVE_POLY[q]
    for seed in range(9000, 9040):
        if graph == "ring":
            code, _, spec = fu.ring_graph(q, poly, seed - 9000)
        else:
            code, _, spec = du.degree_code(q, seed, graph[0], graph[1], graph[2])
        L = frames(code, seed)
        tmp = tempfile.mkdtemp(prefix="golden_")
        df.write_gf_tables(q, os.path.join(tmp, "SRC"), poly)
        du.write_spec_code_file(spec, os.path.join(tmp, "code.txt"))
        L.tofile(os.path.join(tmp, "L_ch.bin"))
        pk = dict(kw, gfq=q, code=os.path.join(tmp, "code.txt"), max_iter=max(iters), parallel=1, crc_len=8, random_msg=0,
                  constellation=REF + "BPSK.txt")
        prof_path = os.path.join(tmp, "profile.txt")
        open(prof_path, "w").write(profile_text(**pk))
        t0 = time.time()
        try:
            subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", f"ref_driver_{build}"), "decode", prof_path, tmp,
                                   os.path.join(tmp, "L_ch.bin"), str(L.shape[0]), ",".join(map(str, iters)), ",".join(map(str, st_iters)), str(lanes)],
                                  cwd=tmp, stderr=subprocess.DEVNULL, stdout=subprocess.DEVNULL, timeout=limit)
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
    arrs["state_lanes"] = np.arange(lanes, dtype=np.int32)
    meta = dict(profile=dict(kw, gfq=q, max_iter=max(iters)), spec=spec, seed=seed, build=build, poly=poly,
                chk_degs=sorted(set(code.chk_deg.tolist())), var_degs=sorted(set(code.var_deg.tolist())),
                reference_flags="-std=c++14 -O2 (NBLDPC.cpp at -%s) -ffp-contract=off, g++ 11.4, x86-64" % build)
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrs)
    shutil.rmtree(tmp)
    print(f"{name}: seed {seed} N={code.N} E={code.E} ret={arrs['ret'].tolist()} syn_ok={arrs['syn_ok'].tolist()} "
          f"(reference {dt:.1f}s, {os.path.getsize(path) / 1e3:.0f} kB)")


FER = {"gf16_m25": (2.0, 8, 64)}     # link shape -> Eb/N0, lanes, Min Sim Cycle (frames)


def run_fer():
    import link_shapes as ls
    from link_util import prepare_spec_workdir
    anchors = {}
    for name, (ebn0, parallel, cycles) in FER.items():
        _, spec, _ = ls.shape(name)
        poly = ls.poly_of(name)
        assert poly is not None and poly != df.PRIMITIVE_POLY[spec["q"]]
        kw = ls.profile_of(name, parallel, snr_begin=ebn0, snr_step=1.0, snr_stop=ebn0, min_sim_cycle=cycles)
        tmp = tempfile.mkdtemp(prefix="golden_")
        prof = prepare_spec_workdir(tmp, kw, spec, ls.points_of(name), absolute=True, poly=poly)
        out = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_driver_O2"), "fer", prof], cwd=tmp, capture_output=True, text=True,
                             check=True, timeout=600).stdout
        shutil.rmtree(tmp)
        pts = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
        for p in pts:
            p.pop("cpu_s", None)
        assert len(pts) == 1 and 0 < pts[0]["errFrame"] < pts[0]["frames"], (name, pts)
        anchors[name] = dict(shape=name, poly=poly, profile=kw, points=pts)
        print(f"fer {name}: {pts}", flush=True)
    with open(os.path.join(GOLD, "fer_anchors_fields.json"), "w") as f:
        json.dump(anchors, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    for n in sys.argv[1:] or list(SETS) + ["fer"]:
        run_fer() if n == "fer" else run_set(n)
