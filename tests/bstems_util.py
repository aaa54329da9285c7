"""Helpers of the BS-TEMS (decode method 7) tests: build and run the CPU checker tests/bstems_check.cpp, synthetic codes, and the
decoder parameters of a golden profile."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LITERAL, CANONICAL = 0, 1


def build_checker(outdir):
    exe = os.path.join(str(outdir), "bstems_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tests", "bstems_check.cpp"),
                           "-o", exe])
    return exe


def bs_kwargs(profile):
    """bs_nm / bs_nc / bs_factor / bs_offset of a golden profile, with the defaults of nbldpc_amd/profiles.py."""
    from nbldpc_amd.profiles import DEFAULTS
    p = dict(DEFAULTS)
    p.update(profile)
    return dict(bs_nm=p["bs_nm"], bs_nc=p["bs_nc"], bs_factor=p["bs_factor"], bs_offset=p["bs_offset"])


def run_checker(exe, code, L_ch, max_iter, mode, bs_nm, bs_nc, bs_factor=1.0, bs_offset=0.0, fixed_iters=0, state=(), threads=None,
                gf=None):
    """code: an nbldpc_amd.Code.  Returns (out [B][N], ret [B], iters [B], {b: (post, v2c, c2v)} for b in `state`)."""
    import nbldpc_amd as nb
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    B, N, w = L_ch.shape
    q, E = code.q, code.E
    assert N == code.N and w == q - 1
    mul, inv = gf if gf is not None else nb.datafiles.gf_tables(q)
    state = [int(b) for b in state]
    hdr = np.array([N, code.M, q, E, bs_nm, bs_nc, max_iter, mode, fixed_iters, B, len(state), 0], dtype=np.int32)
    if threads is None:
        threads = min(16, os.cpu_count() or 1, max(1, B))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(hdr.tobytes())
            f.write(np.array([bs_factor, bs_offset], dtype=np.float64).tobytes())
            for a in (code.var_deg, code.chk_deg, code.var_chk, code.var_h, code.chk_var, code.chk_h):
                f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
            f.write(np.array(mul, dtype=np.int32).reshape(-1).tobytes())
            f.write(np.array(inv, dtype=np.int32).reshape(-1).tobytes())
            f.write(np.array(state, dtype=np.int32).tobytes())
            f.write(L_ch.tobytes())
        subprocess.check_call([exe, fin, fout, str(threads)])
        raw = open(fout, "rb").read()
    o = 0
    out = np.frombuffer(raw, np.int32, B * N, o).reshape(B, N)
    o += 4 * B * N
    ret = np.frombuffer(raw, np.int32, B, o)
    o += 4 * B
    its = np.frombuffer(raw, np.int32, B, o)
    o += 4 * B
    st = {}
    for b in state:
        post = np.frombuffer(raw, np.float64, N * w, o).reshape(N, w)
        o += 8 * N * w
        v2c = np.frombuffer(raw, np.float64, E * w, o).reshape(E, w)
        o += 8 * E * w
        c2v = np.frombuffer(raw, np.float64, E * w, o).reshape(E, w)
        o += 8 * E * w
        st[b] = (post, v2c, c2v)
    assert o == len(raw)
    return out, ret, its, st


def ring_code(q, M, dc):
    """A synthetic (2, dc)-regular graph (dc even): M checks, N = M dc / 2 variables; variable n joins checks n % M and
    (n % M + 1 + n // M) % M (the construction of tests/test_abi.py)."""
    import nbldpc_amd as nb
    assert dc % 2 == 0 and M > dc // 2
    N = M * dc // 2
    chk_rows = [[] for _ in range(M)]
    var_rows = [[] for _ in range(N)]
    for n in range(N):
        for m in (n % M, (n % M + 1 + n // M) % M):
            h = 1 + (7 * n + 3 * m) % (q - 1)
            var_rows[n].append((m + 1, h))
            chk_rows[m].append((n + 1, h))
    return nb.Code(spec=dict(N=N, M=M, q=q, var_rows=var_rows, chk_rows=chk_rows))
