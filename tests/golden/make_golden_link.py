#!/usr/bin/env python3
"""Generate the link_shape_*.npz fixtures and fer_anchors_link.json: the COMPILED REFERENCE's own link chain (oracle/_ref, see
oracle/Makefile `make ref`) on the synthetic transmitter shapes of tests/link_shapes.py.

Build-container only, like make_golden.py; needs everything __graft_entry__.build() makes: oracle/_ref, and the device and host
libraries (nbldpc_amd/csrc, then nbldpc_amd/host), whose GenPN gives the register's period of the stride cases.  Per shape a work
directory is written -- the graph as a reference-format code file (degree_util.write_spec_code_file), the GF tables, the constellation file (BPSK, or the grid of link_shapes.grid_points for the q-ary
shapes) and a profile -- and `ref_driver dump` runs CSimulation / CComm of the unmodified reference in it: FRAMES frames x LANES lanes.
  link_shape_<id>.npz          tx_code [B][N], tx_msg [B][K], sigma [P], L_ch [B][N][q-1] (b = frame * P + lane), and in `meta` the
                               profile, the graph (`spec`), the constellation points and Eb/N0
  link_shape_stride_<k>.npz    the smallest shape with `parallel` = period - 1, period, period + 1 and 2 period of the PN register
                               (link_shapes.pn_period): symbols as bytes, L_ch of the first STRIDE_LCH_LANES lanes of frame 0 only
  fer_anchors_link.json        FER rows of `ref_driver fer` for link_shapes.FER_SHAPES: a few hundred frames at one Eb/N0, chosen so
                               that the reference's row has error frames and error-free frames (asserted here)
The files are written with fixed time stamps: a second run gives the same bytes.

usage: python tests/golden/make_golden_link.py [id ... | stride | fer]      (no argument: everything)
"""
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import link_shapes as ls  # noqa: E402
from link_util import prepare_spec_workdir  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver_O2")
GOLD = os.path.join(ROOT, "tests", "golden")
FRAMES, LANES, EBN0 = 3, 3, 3.0
STRIDE_FRAMES, STRIDE_LCH_LANES = 2, 4
# shape -> (Eb/N0, lanes, Min Sim Cycle = frames, profile overrides) of its FER row.  The q-ary row sends the all-zero message, as every
# shipped QAM anchor does: the reference's modulator packs a symbol's bits MSB first and its demodulator takes the point index as the
# symbol, so with a random message over q points no frame ever decodes (328 error frames of 328 at every Eb/N0 from 4 to 14 dB).  The
# random message over q points is in the shape's chain fixture.
FER = {"exchange_msg": (2.0, 8, 320, {}), "qary_gf8_punct": (4.0, 8, 320, dict(random_msg=0)), "gf8_odd": (3.0, 8, 320, {})}
FLAGS = "-std=c++14 -O2 -ffp-contract=off, g++ 11.4, x86-64"


def save_npz(path, **arrays):
    """np.savez_compressed with fixed time stamps and a fixed member order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def dump(name, parallel, frames, ebn0):
    """the reference's chain on a shape: (arrays of ref_driver dump, profile keys, spec, points)"""
    _, spec, _ = ls.shape(name)
    points = ls.points_of(name)
    kw = ls.profile_of(name, parallel)
    tmp = tempfile.mkdtemp(prefix="golden_")
    prof = prepare_spec_workdir(tmp, kw, spec, points, absolute=True, poly=ls.poly_of(name))
    subprocess.check_call([DRIVER, "dump", prof, tmp, repr(ebn0), str(frames), "1", ""], cwd=tmp, stderr=subprocess.DEVNULL,
                          stdout=subprocess.DEVNULL, timeout=600)
    arrs = {k: np.load(os.path.join(tmp, k + ".npy")) for k in ("tx_code", "tx_msg", "sigma", "L_ch")}
    shutil.rmtree(tmp)
    return arrs, kw, spec, points


def run_shape(name):
    t0 = time.time()
    arrs, kw, spec, points = dump(name, LANES, FRAMES, EBN0)
    meta = dict(shape=name, profile=kw, spec=spec, points=points.tolist(), ebn0=EBN0, frames=FRAMES, reference_flags=FLAGS)
    if ls.poly_of(name) is not None:   # the GF tables of the work directory were written with this modulus
        meta["poly"] = ls.poly_of(name)
    path = os.path.join(GOLD, f"link_shape_{name}.npz")
    save_npz(path, meta=json.dumps(meta), **arrs)
    print(f"link_shape_{name}: N={spec['N']} B={arrs['tx_code'].shape[0]} ({time.time() - t0:.1f}s, {os.path.getsize(path) / 1e3:.0f} kB)", flush=True)


def run_stride():
    for tag, parallel in ls.stride_cases().items():
        t0 = time.time()
        arrs, kw, spec, points = dump(ls.SMALLEST, parallel, STRIDE_FRAMES, EBN0)
        assert arrs["tx_code"].max() < 256
        out = dict(tx_code=arrs["tx_code"].astype(np.uint8), tx_msg=arrs["tx_msg"].astype(np.uint8), sigma=arrs["sigma"][:1],
                   L_ch=arrs["L_ch"][:STRIDE_LCH_LANES])
        meta = dict(shape=ls.SMALLEST, profile=kw, spec=spec, points=points.tolist(), ebn0=EBN0, frames=STRIDE_FRAMES,
                    lch_lanes=STRIDE_LCH_LANES, reference_flags=FLAGS)
        path = os.path.join(GOLD, f"link_shape_stride_{tag}.npz")
        save_npz(path, meta=json.dumps(meta), **out)
        print(f"link_shape_stride_{tag}: parallel={parallel} ({time.time() - t0:.1f}s, {os.path.getsize(path) / 1e3:.0f} kB)", flush=True)


def run_fer():
    anchors = {}
    for name, (ebn0, parallel, cycles, over) in FER.items():
        _, spec, _ = ls.shape(name)
        kw = ls.profile_of(name, parallel, snr_begin=ebn0, snr_step=1.0, snr_stop=ebn0, min_sim_cycle=cycles, **over)
        tmp = tempfile.mkdtemp(prefix="golden_")
        prof = prepare_spec_workdir(tmp, kw, spec, ls.points_of(name), absolute=True)
        t0 = time.time()
        out = subprocess.run([DRIVER, "fer", prof], cwd=tmp, capture_output=True, text=True, check=True, timeout=600).stdout
        shutil.rmtree(tmp)
        pts = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
        for p in pts:
            p.pop("cpu_s", None)
        assert len(pts) == 1 and 0 < pts[0]["errFrame"] < pts[0]["frames"], (name, pts)   # error frames and error-free frames
        anchors[name] = dict(shape=name, profile=kw, points=pts)
        print(f"fer {name}: {pts} ({time.time() - t0:.1f}s)", flush=True)
    with open(os.path.join(GOLD, "fer_anchors_link.json"), "w") as f:
        json.dump(anchors, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    for a in sys.argv[1:] or [n for n in ls.SHAPES if n not in ls.NO_REFERENCE] + ["stride", "fer"]:
        if a == "stride":
            run_stride()
        elif a == "fer":
            run_fer()
        else:
            run_shape(a)
