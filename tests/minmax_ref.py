"""Min-Max decoding (method 3, nbl_create_minmax) as include/nbldpc.h defines it, restated in numpy -- TEST INFRASTRUCTURE ONLY.

The check node is the header's five steps; between its two rounded subtractions there is only min and max, which select and never
round, so the result is a property of the configuration SET and every correct evaluation gives the same bits: the GPU is held to
np.array_equal, and tests/test_minmax.py holds the recursion here to the brute-force minimum over all configurations.  The flooding
iteration is the EMS iteration of the reference (post in the variable's edge order, decision, syndrome, the freeze at the first zero
syndrome, v2c = post - c2v, no damping); the layered one is tests/layered_ref.py's, which takes the check node through an object that
offers .code and .check(m, vin)."""
import itertools

import numpy as np

import layered_ref as lr


def shape(y, factor, offset):
    """the library's shaping of a c2v value, as EMS applies it"""
    y = np.asarray(y, dtype=np.float64)
    if factor == 1.0 and offset == 0.0:
        return np.where((y < 0.0) | (y > 0.0), y, 0.0)
    if factor != 1.0:
        y = y / factor
    return np.where(y < -1 * offset, y + offset, np.where(y > offset, y - offset, 0.0))


def dissimilarities(vin, h, mul):
    """steps 1 and 2: vin [dc][q-1], h [dc] -> u [dc][q] in the check domain"""
    dc, q = vin.shape[0], vin.shape[1] + 1
    u = np.zeros((dc, q))
    for d in range(dc):
        p = np.zeros(q)
        p[mul[h[d], 1:]] = vin[d]
        u[d] = p.max() - p
    return u


def step(A, B):
    """E(A,B)[c] = min_a max(A[a], B[a ^ c])"""
    q = A.shape[0]
    idx = np.arange(q)[:, None] ^ np.arange(q)[None, :]
    return np.min(np.maximum(A[None, :], B[idx]), axis=1)


def combine(u):
    """step 3 by the forward / backward recursion: u [dc][q] -> w [dc][q]"""
    dc = u.shape[0]
    if dc == 2:
        return np.array([u[1], u[0]])
    F = {1: u[0]}
    for k in range(1, dc - 1):
        F[k + 1] = step(F[k], u[k])
    R = {dc - 2: u[dc - 1]}
    for k in range(dc - 2, 0, -1):
        R[k - 1] = step(R[k], u[k])
    return np.array([R[0] if d == 0 else F[dc - 1] if d == dc - 1 else step(F[d], R[d]) for d in range(dc)])


def combine_brute(u):
    """step 3 as it is defined: the minimum over every configuration of the other edges"""
    dc, q = u.shape
    w = np.full((dc, q), np.inf)
    for d in range(dc):
        others = [k for k in range(dc) if k != d]
        for conf in itertools.product(range(q), repeat=dc - 1):
            y = 0
            for a in conf:
                y ^= a
            w[d, y] = min(w[d, y], max(u[k, a] for k, a in zip(others, conf)))
    return w


def outputs(w, h, mul, factor=1.0, offset=0.0):
    """steps 4 and 5: w [dc][q] -> c2v [dc][q-1]"""
    dc, q = w.shape
    out = np.zeros((dc, q - 1))
    for d in range(dc):
        c = w[d, 0] - w[d]
        out[d] = shape(c[mul[h[d], 1:]], factor, offset)
    return out


def check_node(vin, h, mul, factor=1.0, offset=0.0, brute=False):
    u = dissimilarities(np.asarray(vin, dtype=np.float64), h, mul)
    return outputs(combine_brute(u) if brute else combine(u), h, mul, factor, offset)


class _Code:
    """the graph of an nbldpc_amd.Code in the form tests/layered_ref.py's Graph reads"""

    def __init__(self, code):
        self.N, self.M, self.E, self.q = code.N, code.M, code.E, code.q
        voff = np.concatenate([[0], np.cumsum(code.var_deg)])
        coff = np.concatenate([[0], np.cumsum(code.chk_deg)])
        v_k = np.zeros(code.E, dtype=np.int64)
        c2e = np.zeros(code.E, dtype=np.int64)
        for n in range(code.N):
            for e in range(voff[n], voff[n + 1]):
                m = code.var_chk[e]
                ks = [k for k in range(code.chk_deg[m]) if code.chk_var[coff[m] + k] == n]
                assert len(ks) == 1, "a variable joins a check once"
                v_k[e] = ks[0]
                c2e[coff[m] + ks[0]] = e
        self._arr = dict(dv=code.var_deg, dc=code.chk_deg, v_chk=code.var_chk, v_k=v_k, c_var=code.chk_var, c_h=code.chk_h, c2e=c2e)

    def arr(self, name, n):
        a = np.asarray(self._arr[name])
        assert a.shape == (n,)
        return a


class MinMax:
    """.code and .check(m, vin): what tests/layered_ref.py's decode asks of a decoder"""

    def __init__(self, code, mul, factor=1.0, offset=0.0):
        self.code, self.mul, self.factor, self.offset = _Code(code), np.asarray(mul), factor, offset
        self.g = lr.Graph(self.code)

    def check(self, m, vin):
        g = self.g
        return check_node(vin, g.c_h[g.coff[m]:g.coff[m + 1]], self.mul, self.factor, self.offset)


def decode_flooding(mm, L_ch, max_iter, fixed_iters=0):
    """One frame under the flooding schedule.  Returns out [N], converged, iters, post [N][q-1], c2v [E][q-1] (variable-major edge order,
    as nbl_read_state returns it)."""
    g = mm.g
    w = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    c2v = np.zeros((g.E, w))                             # check-major
    v2c = np.zeros((g.E, w))                             # variable-major
    post = np.zeros((g.N, w))
    out = np.zeros(g.N, dtype=np.int32)
    frozen, iters = 0, max_iter
    for it in range(1, max_iter + 1):
        dec = np.zeros(g.N, dtype=np.int32)
        for n in range(g.N):
            P = L_ch[n].copy()
            for e in range(g.voff[n], g.voff[n + 1]):
                P = P + c2v[g.v_slot[e]]
            post[n] = P
            dec[n] = lr._decide(P)
            for e in range(g.voff[n], g.voff[n + 1]):
                v2c[e] = P - c2v[g.v_slot[e]]
        if not frozen:
            out = dec.copy()
        ok = True
        for m in range(g.M):
            s = 0
            for ce in range(g.coff[m], g.coff[m + 1]):
                s ^= int(mm.mul[g.c_h[ce], dec[g.c_var[ce]]])
            ok = ok and s == 0
        if ok and not frozen:
            frozen, iters = 1, it
            if not fixed_iters:
                break
        new = np.zeros_like(c2v)
        for m in range(g.M):
            sl = slice(g.coff[m], g.coff[m + 1])
            new[sl] = mm.check(m, v2c[g.c2e[sl]])
        c2v = new
    c2v_vm = np.zeros_like(c2v)
    c2v_vm[g.c2e] = c2v
    return out, frozen, iters, post.copy(), c2v_vm


def decode(mm, L_ch, layer_of, max_iter, fixed_iters=0):
    """layer_of None: flooding; else the layered schedule with that assignment"""
    if layer_of is None:
        return decode_flooding(mm, L_ch, max_iter, fixed_iters)
    return lr.decode(mm, mm.mul, L_ch, layer_of, max_iter, fixed_iters=fixed_iters)
