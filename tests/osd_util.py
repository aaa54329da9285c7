"""Helpers of the OSD tests: build and run the CPU checker tests/osd_check.cpp, the reference's symbol decision, and the decoder
parameters of a golden profile."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(outdir):
    exe = os.path.join(str(outdir), "osd_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "osd_check.cpp"), "-o", exe])
    return exe


def profile(meta):
    from nbldpc_amd.profiles import DEFAULTS
    p = dict(DEFAULTS)
    p.update(meta["profile"])
    return p


def osd_kwargs(p):
    """Decoder keyword arguments of a golden profile's OSD / CRC fields."""
    return dict(osd_order=p["osd_order"], osd_flag=p["osd_flag"], osd_factor=p["osd_factor"], crc_len=p["crc_len"],
                crc_rows=p["crc_correct"])


def decide(post):
    """DecideLLRVector over the last axis ([..][q-1]): the first strict maximum above 0 (symbol index + 1), else 0."""
    mx = post.max(axis=-1)
    return np.where(mx > 0, post.argmax(axis=-1) + 1, 0).astype(np.int32)


COUNTERS = ("rotations", "repairs", "max_rot", "flips", "differs", "nd_bit", "best")


def run_checker(exe, code, L_ch, order, flag=1, crc_len=8, crc_rows=0, gf_mat=None, S=None, base=None, counters=False):
    """OSD of every codeword of L_ch [B][N][q-1]; flag 0 takes S [B][N p] and base [B][N].  Returns out [B][N]; with counters=True
    also the checker's per-frame counters as a dict of [B] arrays (COUNTERS, described at the head of tests/osd_check.cpp)."""
    import nbldpc_amd as nb
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    B, N, w = L_ch.shape
    q = code.q
    assert N == code.N and w == q - 1
    gm = nb.datafiles.gf_matrices(q) if gf_mat is None else gf_mat
    hdr = np.array([N, code.M, q, code.E, order, flag, B, crc_len, crc_rows], dtype=np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(hdr.tobytes())
            for a in (code.var_deg, code.var_chk, code.var_h):
                f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(gm, dtype=np.uint8).tobytes())
            f.write(L_ch.tobytes())
            if not flag:
                f.write(np.ascontiguousarray(S, dtype=np.float64).tobytes())
                f.write(np.ascontiguousarray(base, dtype=np.int32).tobytes())
        if not counters:
            subprocess.check_call([exe, fin, fout])
            return np.fromfile(fout, dtype=np.int32).reshape(B, N)
        fcnt = os.path.join(tmp, "cnt.bin")
        subprocess.check_call([exe, fin, fout, fcnt])
        c = np.fromfile(fcnt, dtype=np.float64).reshape(B, len(COUNTERS))
        return np.fromfile(fout, dtype=np.int32).reshape(B, N), {k: c[:, i] for i, k in enumerate(COUNTERS)}


def flag0_sums(posts, factor):
    """S after T = len(posts) iterations: S_t = factor * S_(t-1) + post_t[n][2^k - 1], S_0 = 0 (NBLDPC.cpp:687), as [N p]."""
    N, w = posts[0].shape
    p = (w + 1).bit_length() - 1
    S = np.zeros(N * p)
    for P in posts:
        S = factor * S + P[:, [(1 << k) - 1 for k in range(p)]].reshape(-1)
    return S
