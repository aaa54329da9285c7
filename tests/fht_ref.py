"""FHT sum-product decoding (include/nbldpc.h, nbl_create_fht) restated in numpy -- TEST INFRASTRUCTURE ONLY.

check_node() is the header's check-node update, step by step, generic in dtype: np.float64 is the restatement the kernels are compared
with, np.longdouble (80-bit on x86) measures how far a rounding can move the result.  FhtCheck wraps it as an object with .code and
.check(m, vin), so that layered_bp_ref.decode runs the layered schedule on it unchanged (FP64); decode_layered() is the same schedule
generic in dtype (tests/test_fht.py holds the two equal bit for bit in FP64), decode_flooding() the reference's log-QSPA iteration
(NBLDPC.cpp:643-775) around that check, with the per-edge 0.5 / 0.5 damping, the freeze rules and fixed_iters as layered_bp_ref.decode
has them.  State is returned as nbl_read_state returns it: under flooding a frame that converged at iteration k holds the v2c of
iteration k (the variable-node pass precedes the syndrome on the GPU, include/nbldpc.h at nbl_read_state) and the c2v of iteration k-1.

w(x) = exp(x - max x), the implicit 0 of slot 0 included, is the probability-domain view the parity statement is made in.

D80: per case of tests/test_gpu_fht.py the largest |w(x_fp64) - w(x_80bit)| over post, c2v and v2c of every frame, recorded from
tests/test_fht.py::test_conditions_on_every_gpu_case (which recomputes and compares it).  The GPU tolerance is 16 x this figure."""
import numpy as np

from layered_ref import Graph, _decide
from layered_bp_ref import _gap

FLOOR_LOG2 = 40  # NBL_FHT_FLOOR_LOG2

# (case, schedule) -> D80; "fixed" = gf16 with fixed_iters = 1; schedules: flooding, and the layer assignments the GPU tests use
D80 = {
    ("gf16", "flooding"): 2.385e-14,
    ("gf16", "greedy"): 4.917e-14,
    ("ring256", "flooding"): 1.889e-13,
    ("ring256", "greedy"): 7.253e-13,
    ("ring256", "serial"): 4.328e-13,
    ("ring256", "other"): 6.553e-12,
    ("ring64", "flooding"): 1.411e-12,
    ("ring64", "greedy"): 5.436e-12,
    ("ring64", "serial"): 2.227e-12,
    ("ring64", "other"): 1.699e-12,
    ("all-4", "flooding"): 1.194e-14,
    ("all-4", "greedy"): 2.132e-14,
    ("all-8", "flooding"): 1.244e-11,
    ("all-8", "greedy"): 1.254e-12,
    ("all-16", "flooding"): 1.307e-12,
    ("all-16", "greedy"): 9.555e-12,
    ("dv48-32", "flooding"): 1.284e-13,
    ("dv48-32", "greedy"): 1.247e-12,
    ("rand128", "flooding"): 7.365e-14,
    ("rand128", "greedy"): 3.221e-14,
    ("gf16-fixed", "flooding"): 2.211e-14,
    ("gf16-fixed", "greedy"): 1.741e-13,
}


def wht(x):
    """unnormalised Walsh-Hadamard transform along the last axis: strides 1, 2, .., q/2, (x[i], x[i+s]) <- (x[i] + x[i+s], x[i] - x[i+s])"""
    q = x.shape[-1]
    s = 1
    while s < q:
        y = x.reshape(x.shape[:-1] + (q // (2 * s), 2, s))
        x = np.stack([y[..., 0, :] + y[..., 1, :], y[..., 0, :] - y[..., 1, :]], axis=-2).reshape(x.shape)
        s *= 2
    return x


def check_node(vin, h, gf_mul, dtype=np.float64, floor=True):
    """vin [dc][q-1] incoming LLR vectors (slot 0 implicit), h [dc] edge coefficients, gf_mul [q][q].  Returns c2v [dc][q-1] in `dtype`.
    floor=False leaves step 6 out (only to show what it does)."""
    dc, q = len(h), gf_mul.shape[0]
    perm = np.asarray(gf_mul)[np.asarray(h, dtype=np.int64)].astype(np.int64)  # perm[d][a] = h_d a
    p = np.zeros((dc, q), dtype=dtype)
    for d in range(dc):
        p[d, perm[d, 1:]] = np.asarray(vin[d], dtype=dtype)                   # 1.
    u = np.exp(p - p.max(axis=1, keepdims=True))                              # 2.
    U = wht(u)                                                                # 3.
    fwd, bwd = [None] * dc, [None] * dc                                       # 4.
    fwd[1] = U[0]
    for k in range(1, dc - 1):
        fwd[k + 1] = fwd[k] * U[k]
    bwd[dc - 2] = U[dc - 1]
    for k in range(dc - 2, 0, -1):
        bwd[k - 1] = bwd[k] * U[k]
    V = np.stack([bwd[0] if d == 0 else fwd[d] if d == dc - 1 else fwd[d] * bwd[d] for d in range(dc)])
    v = wht(V)                                                                # 5.
    if floor:
        t = v.max(axis=1, keepdims=True)                                      # 6.
        assert np.all(t > 0)
        v = np.maximum(v, t * dtype(2.0) ** -FLOOR_LOG2)
    c = np.log(v) - np.log(v[:, :1])                                          # 7.
    return np.stack([c[d, perm[d, 1:]] for d in range(dc)])


def brute_force(vin, h, gf_mul):
    """The exact box-plus by direct XOR convolution in 80-bit arithmetic: c2v [dc][q-1] (np.longdouble), no floor."""
    dc, q = len(h), gf_mul.shape[0]
    perm = np.asarray(gf_mul)[np.asarray(h, dtype=np.int64)].astype(np.int64)
    p = np.zeros((dc, q), dtype=np.longdouble)
    for d in range(dc):
        p[d, perm[d, 1:]] = np.asarray(vin[d], dtype=np.longdouble)
    u = np.exp(p - p.max(axis=1, keepdims=True))
    xor = np.arange(q)[:, None] ^ np.arange(q)[None, :]
    out = []
    for d in range(dc):
        acc = None
        for k in range(dc):
            if k != d:
                acc = u[k] if acc is None else (acc[None, :] * u[k][xor]).sum(axis=1)  # acc'[b] = sum_x acc[x] u_k[b ^ x]
        c = np.log(acc) - np.log(acc[0])
        out.append(c[perm[d, 1:]])
    return np.stack(out)


def w(x):
    """rows of LLRs [n][q-1] -> probabilities relative to the largest, [n][q], the implicit 0 of slot 0 included"""
    x = np.asarray(x)
    full = np.concatenate([np.zeros(x.shape[:-1] + (1,), dtype=x.dtype), x], axis=-1)
    return np.exp(full - full.max(axis=-1, keepdims=True))


def w_dev(a, b):
    """largest |w(a) - w(b)| (as np.float64)"""
    return float(np.max(np.abs(w(np.asarray(a, dtype=np.longdouble)) - w(np.asarray(b, dtype=np.longdouble)))))


class FhtCheck:
    """What layered_bp_ref.decode needs of a decoder: .code (a pyoracle.Code) and .check(m, vin) -> c2v [dc][q-1]"""

    def __init__(self, ocode, gf_mul, dtype=np.float64):
        self.code, self.g, self.mul, self.dtype = ocode, Graph(ocode), np.asarray(gf_mul), dtype

    def check(self, m, vin):
        g = self.g
        return check_node(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul, self.dtype)


def _post(g, L_ch, c2v, n):
    P = L_ch[n].copy()
    for e in range(g.voff[n], g.voff[n + 1]):
        P = P + c2v[g.v_slot[e]]
    return P


def _syndrome_ok(g, gf_mul, dec):
    for m in range(g.M):
        s = 0
        for ce in range(g.coff[m], g.coff[m + 1]):
            s ^= int(gf_mul[g.c_h[ce], dec[g.c_var[ce]]])
        if s:
            return False
    return True


def _finish(g, out, frozen, iters, post, c2v, v2c, gap):
    c2v_vm, v2c_vm = np.zeros_like(c2v), np.zeros_like(v2c)
    c2v_vm[g.c2e] = c2v
    v2c_vm[g.c2e] = v2c
    return out, frozen, iters, post.copy(), c2v_vm, v2c_vm, gap


def decode_flooding(chk, L_ch, max_iter, fixed_iters=0):
    """One frame under the flooding schedule.  chk: FhtCheck (its dtype is the arithmetic of the whole decode).
    Returns out [N], converged, iters, post, c2v, v2c (variable-major edge order) and the smallest decide gap."""
    g, dt, mul = chk.g, chk.dtype, chk.mul
    wd = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=dt)
    c2v = np.zeros((g.E, wd), dtype=dt)                  # check-major
    v2c = L_ch[g.c_var].copy()                           # check-major (NBLDPC.cpp:647-655)
    post = np.zeros((g.N, wd), dtype=dt)
    out = np.zeros(g.N, dtype=np.int32)
    frozen, iters, gap = 0, max_iter, np.inf
    half = dt(0.5)
    for it in range(1, max_iter + 1):
        dec = np.zeros(g.N, dtype=np.int32)
        for n in range(g.N):
            P = _post(g, L_ch, c2v, n)
            post[n] = P
            dec[n] = _decide(P)
            gap = min(gap, _gap(P))
            for e in range(g.voff[n], g.voff[n + 1]):    # the variable-node pass (:718-744), before the syndrome as on the GPU
                ce = g.v_slot[e]
                raw, old = P - c2v[ce], v2c[ce]
                gap = min(gap, _gap(raw), _gap(old))
                if _decide(raw) != _decide(old):
                    raw = half * old + half * raw        # two rounded products, one rounded sum
                v2c[ce] = raw
        if not frozen:
            out = dec.copy()
        if _syndrome_ok(g, mul, dec) and not frozen:
            frozen, iters = 1, it
            if not fixed_iters:
                break
        for m in range(g.M):
            c2v[g.coff[m]:g.coff[m + 1]] = chk.check(m, v2c[g.coff[m]:g.coff[m + 1]])
    return _finish(g, out, frozen, iters, post, c2v, v2c, gap)


def decode_layered(chk, L_ch, layer_of, max_iter, fixed_iters=0):
    """One frame under the layered schedule: layered_bp_ref.decode generic in dtype.  Same return as decode_flooding."""
    g, dt, mul = chk.g, chk.dtype, chk.mul
    wd = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=dt)
    order = [m for l in range(int(max(layer_of)) + 1) for m in range(g.M) if layer_of[m] == l]
    assert sorted(order) == list(range(g.M))
    c2v = np.zeros((g.E, wd), dtype=dt)
    v2c = L_ch[g.c_var].copy()
    post = np.zeros((g.N, wd), dtype=dt)
    out = np.zeros(g.N, dtype=np.int32)
    frozen, iters, gap = 0, max_iter, np.inf
    half = dt(0.5)
    for it in range(1, max_iter + 1):
        dec = np.zeros(g.N, dtype=np.int32)
        for n in range(g.N):
            P = _post(g, L_ch, c2v, n)
            post[n] = P
            dec[n] = _decide(P)
            gap = min(gap, _gap(P))
        if not frozen:
            out = dec.copy()
        if _syndrome_ok(g, mul, dec) and not frozen:
            frozen, iters = 1, it
            if not fixed_iters:
                break
        for m in order:
            vin = np.zeros((g.dc[m], wd), dtype=dt)
            for k in range(g.dc[m]):
                ce = g.coff[m] + k
                raw = _post(g, L_ch, c2v, g.c_var[ce]) - c2v[ce]     # the CURRENT values
                old = v2c[ce]
                gap = min(gap, _gap(raw), _gap(old))
                if _decide(raw) != _decide(old):
                    raw = half * old + half * raw
                v2c[ce] = raw
                vin[k] = raw
            c2v[g.coff[m]:g.coff[m + 1]] = chk.check(m, vin)
    return _finish(g, out, frozen, iters, post, c2v, v2c, gap)


def decode(chk, L_ch, layer_of, max_iter, fixed_iters=0):
    """layer_of None = flooding"""
    if layer_of is None:
        return decode_flooding(chk, L_ch, max_iter, fixed_iters)
    return decode_layered(chk, L_ch, layer_of, max_iter, fixed_iters)


def state_dev(a, b):
    """largest probability-domain deviation between two results of decode() over post, c2v and v2c"""
    return max(w_dev(a[k], b[k]) for k in (3, 4, 5))
