"""The decoder grid of tests/test_gpu_soft.py, its frames and its CPU references -- TEST INFRASTRUCTURE ONLY, shared with
tests/test_soft.py, which measures the restatement's own log-sum error on the same inputs.

Frames are the host link chain's (hostlib.frontend: random message, encoder, BPSK, AWGN), a few lanes at each of three Eb/N0 points, so
that under early exit a case holds frames that converge at iteration 1 (the shared zero block), at an even and at an odd iteration
>= 3 (both c2v buffers) and at least two that never converge.  The points and seeds were chosen on the CPU with the oracle; has_mix()
is asserted on the oracle's flags inside every early-exit test.
"""
import functools
import tempfile

import numpy as np

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib
import layered_ref as lr
import layered_tems_ref as ltr
from degree_util import profile_code
from test_layered import oracle_edges

U16, U256, BDS = "divsalar.UNBLDPC.128.64.GF.16", "divsalar.UNBLDPC.128.64.GF.256", "BDS.576.288.GF.64"

# graph -> (Eb/N0 points, lanes taken at each, seed)
FRAMES = {
    U16: ((9.0, 4.0, 1.0), (8, 8, 8), 173),
    U256: ((9.0, 4.0, 1.0), (8, 8, 8), 173),
    BDS: ((10.0, 3.0, 0.0), (3, 3, 2), 173),
    "all4": ((20.0, 12.0, 4.0), (8, 8, 8), 5),          # rate 1/8 graphs of 16 symbols: the points sit that much higher
    "all8": ((20.0, 12.0, 4.0), (8, 8, 8), 5),
    "all64": ((20.0, 12.0, 4.0), (8, 8, 8), 5),
}

# method name -> (nb method, decoder kwargs by graph); T-EMS runs 6 iterations (its CPU oracle is slow at GF(256)), the others 8
EMS_KW = {U16: dict(ems_nm=8, ems_nc=3), U256: dict(ems_nm=16, ems_nc=3), BDS: dict(ems_nm=16, ems_nc=3),
          "all4": dict(ems_nm=2, ems_nc=3), "all8": dict(ems_nm=4, ems_nc=3), "all64": dict(ems_nm=32, ems_nc=3)}
TEMS_KW = dict(tems_nr=2, tems_nc=3)
BS_KW = dict(bs_nm=4, bs_nc=2)
MODES = {"poll0": dict(fixed_iters=0, poll_every=0), "poll2": dict(fixed_iters=0, poll_every=2), "fixed": dict(fixed_iters=1)}


def max_iter_of(method):
    return 6 if method in ("tems", "tems_layered") else 8


@functools.lru_cache(maxsize=None)
def graph(name):
    """(nb.Code, oracle edge tuple, spec or None)"""
    if name.startswith("all"):
        return profile_code("all", int(name[3:]))
    code = nb.Code(name)
    return code, oracle_edges(code), None


@functools.lru_cache(maxsize=None)
def frames(name):
    """L_ch [B][N][q-1] of a graph's frames, and the per-bit LLRs lam [B][N p] they were expanded from (Comm.cpp:356:
    -2 rx / sigma^2; these profiles puncture nothing)"""
    ebn0s, lanes, seed = FRAMES[name]
    code, _, spec = graph(name)
    N, K, q, P = code.N, code.N - code.M, code.q, max(lanes)
    p = q.bit_length() - 1
    Ls, lams = [], []
    with tempfile.TemporaryDirectory() as t:
        kw = dict(gfq=q, method=2, max_iter=8, parallel=P, random_msg=1, seed=seed, nqam=2)
        if spec is None:
            hostlib.prepare_workdir(t, dict(kw, code=name, constellation="BPSK"), name, "BPSK")
        else:
            from link_util import prepare_spec_workdir
            pts = np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])])
            prepare_spec_workdir(t, dict(kw, crc_len=0), spec, pts)                  # (K p = 4 message bits at GF(4): no room for a CRC)
        for e, k in zip(ebn0s, lanes):
            L, _, _, sigma = hostlib.frontend(t, e, 1, N, K, q, P)
            rx, _, _, sigma2 = hostlib.channel(t, e, 1, N * p, P)
            assert sigma == sigma2
            Ls.append(L[:k])
            lams.append((-2 * rx[:k, :, 0] / (sigma * sigma)))
    L, lam = np.concatenate(Ls), np.concatenate(lams)
    L.setflags(write=False)
    lam.setflags(write=False)
    return L, lam


def has_mix(conv, its):
    """one frame converged at iteration 1, one at an even iteration, one at an odd iteration >= 3, two or more never"""
    c = [int(i) for f, i in zip(conv, its) if f]
    return (1 in c and any(i % 2 == 0 for i in c) and any(i % 2 == 1 and i >= 3 for i in c) and sum(1 for f in conv if not f) >= 2)


def _decide(P):
    return lr._decide(P)


@functools.lru_cache(maxsize=None)
def _checker():
    import atexit
    import shutil
    import bstems_util as bu
    d = tempfile.mkdtemp(prefix="nbl_soft_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return bu.build_checker(d)


@functools.lru_cache(maxsize=None)
def oracle_flags(name, method):
    """(converged [B], iters [B]) of a case under early exit, from the CPU: the canonical oracle (EMS, T-EMS, log-QSPA), the layered
    restatements, the BS-TEMS checker"""
    if method in ("ems", "tems", "ems_layered", "tems_layered", "osd", "ems1100"):
        ref = oracle_state(name, method, 0)                                          # (the sampled frames, where it is a sample)
        return np.array([ref[b][0] for b in sorted(ref)]), np.array([ref[b][1] for b in sorted(ref)])
    import pyoracle as po
    code, edges, _ = graph(name)
    L, _ = frames(name)
    if method == "bstems":
        import bstems_util as bu
        _, ret, its, _ = bu.run_checker(_checker(), code, L, max_iter_of(method), bu.CANONICAL, BS_KW["bs_nm"], BS_KW["bs_nc"])
        return ret.copy(), its.copy()
    assert method == "bp"
    od = po.Decoder(po.Code(edges=edges), po.GF(code.q), po.BP, max_iter_of(method), po.CANONICAL)
    res = [od.decode(L[b]) for b in range(L.shape[0])]
    return np.array([r[0] for r in res]), np.array([r[2] for r in res])


# the T-EMS oracle at GF(256) costs 0.4 s per iteration and frame: its frames are a sample, chosen with that oracle -- frames that
# converge at iteration 1, 2 and 3 and two that never do (under fixed iterations, where every frame costs max_iter: three of them)
U256_TEMS_SAMPLE = (2, 0, 8, 16, 17)


def oracle_sample(name, method, fixed=0):
    if name == U256 and method == "tems":
        return list(U256_TEMS_SAMPLE[::2] if fixed else U256_TEMS_SAMPLE)
    return list(range(frames(name)[0].shape[0]))


@functools.lru_cache(maxsize=None)
def oracle_state(name, method, fixed):
    """{b: (converged, iters, out, c2v [E][q-1] variable-major)} of the frames of oracle_sample(): the bit-exact CPU reference of the
    EMS / T-EMS cases, flooding and layered (greedy layers)"""
    import pyoracle as po
    po.build()
    code, edges, _ = graph(name)
    L, _ = frames(name)
    base = {"ems": "ems", "osd": "ems", "ems1100": "ems", "ems_layered": "ems", "tems": "tems", "tems_layered": "tems"}[method]
    iters = max_iter_of(method)
    kw = EMS_KW[name] if base == "ems" else TEMS_KW
    ocode, gf = po.Code(edges=edges), po.GF(code.q)
    od = po.Decoder(ocode, gf, po.EMS if base == "ems" else po.TEMS, iters, po.CANONICAL, fixed_iters=fixed, **kw)
    out = {}
    if method.endswith("_layered"):
        lay = lr.greedy_layers(code.chk_deg, code.chk_var)
        mod = lr if base == "ems" else ltr
        for b, r in enumerate(mod.decode_batch(od, gf.mul, L, lay, iters, fixed_iters=fixed)):
            out[b] = (int(r[1]), int(r[2]), r[0], r[4])
        return out
    for b in oracle_sample(name, method, fixed):
        r, o, it = od.decode(L[b])
        out[b] = (int(r), int(it), o.copy(), od.state()[2])
    return out


# ---- the grid ------------------------------------------------------------------------------------------------------------------
def decoder(name, method, mode, max_iter=None, **extra):
    """the nb.Decoder of a grid cell"""
    code, _, _ = graph(name)
    it = max_iter_of(method) if max_iter is None else max_iter
    kw = dict(MODES[mode], **extra)
    if method in ("ems", "ems1100"):
        return nb.Decoder(code, nb.METHOD_EMS, it, **EMS_KW[name], **kw)
    if method == "tems":
        return nb.Decoder(code, nb.METHOD_TEMS, it, **TEMS_KW, **kw)
    if method == "bp":
        return nb.Decoder(code, nb.METHOD_BP, it, **kw)
    if method == "bstems":
        return nb.Decoder(code, nb.METHOD_BS_TEMS, it, **BS_KW, **kw)
    if method == "ems_layered":
        return nb.Decoder(code, nb.METHOD_EMS, it, layers="greedy", **EMS_KW[name], **kw)
    if method == "tems_layered":
        return nb.Decoder(code, nb.METHOD_TEMS, it, layers="greedy", damped=True, **TEMS_KW, **kw)
    if method == "osd":
        return nb.Decoder(code, nb.METHOD_EMS, it, osd_order=1, osd_flag=1, **EMS_KW[name], **kw)
    raise KeyError(method)


GRID = ([(U256, m, g) for m in ("ems", "tems", "bp") for g in (0, 1, 2)]
        + [(U16, m, 0) for m in ("ems", "tems", "bp", "bstems", "ems_layered", "tems_layered", "osd")]
        + [(BDS, m, 0) for m in ("ems", "tems", "bp")]
        + [(f"all{q}", m, 0) for q in (4, 8, 64) for m in ("ems", "bp")])
EXACT = ("ems", "tems", "ems_layered", "tems_layered", "osd", "ems1100")   # methods with a bit-exact CPU reference of their c2v
