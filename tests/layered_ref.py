"""The layered (check-serial) EMS schedule of include/nbldpc.h, restated in numpy -- TEST INFRASTRUCTURE ONLY.

A layered iteration is the reference's check-node update applied in another order to messages formed by the reference's own
two expressions (AddLLRVector / MinusLLRVector), so the per-check update is NOT restated here: it is taken from the oracle's
single-check entry point (pyoracle.Decoder(mode=CANONICAL).check, pinned to the compiled reference by
tests/test_oracle_golden.py).  Everything else is a dozen lines of IEEE double adds in the order the header fixes.
"""
import numpy as np


class Graph:
    """The Tanner graph as the oracle holds it (both edge orders), from a pyoracle.Code."""

    def __init__(self, ocode):
        self.N, self.M, self.E, self.q = ocode.N, ocode.M, ocode.E, ocode.q
        self.dv, self.dc = ocode.arr("dv", self.N), ocode.arr("dc", self.M)
        self.voff = np.concatenate([[0], np.cumsum(self.dv)]).astype(np.int64)
        self.coff = np.concatenate([[0], np.cumsum(self.dc)]).astype(np.int64)
        self.v_chk, self.v_k = ocode.arr("v_chk", self.E), ocode.arr("v_k", self.E)
        self.c_var, self.c_h, self.c2e = ocode.arr("c_var", self.E), ocode.arr("c_h", self.E), ocode.arr("c2e", self.E)
        # check-major slot of every variable-major edge: where its c2v vector lives
        self.v_slot = (self.coff[self.v_chk] + self.v_k).astype(np.int64)


def greedy_layers(chk_deg, chk_var):
    """Checks in ascending index, each gets the smallest layer that holds no check sharing a variable with it."""
    off = np.concatenate([[0], np.cumsum(chk_deg)])
    taken = {}                                           # variable -> layers of the checks it has joined
    layer_of = np.zeros(len(chk_deg), dtype=np.int32)
    for m in range(len(chk_deg)):
        vs = [int(v) for v in chk_var[off[m]:off[m + 1]]]
        used = set().union(*(taken.get(v, set()) for v in vs))
        l = 0
        while l in used:
            l += 1
        layer_of[m] = l
        for v in vs:
            taken.setdefault(v, set()).add(l)
    return layer_of


def layers_valid(chk_deg, chk_var, layer_of):
    """Every layer 0 .. max non-empty and no two checks of a layer sharing a variable."""
    off = np.concatenate([[0], np.cumsum(chk_deg)])
    if min(layer_of) < 0 or set(int(x) for x in layer_of) != set(range(int(max(layer_of)) + 1)):
        return False
    seen = set()
    for m in range(len(chk_deg)):
        for v in set(int(v) for v in chk_var[off[m]:off[m + 1]]):
            if (int(layer_of[m]), v) in seen:
                return False
            seen.add((int(layer_of[m]), v))
    return True


def _decide(P):
    """DecideLLRVector (NBLDPC.cpp:1542-1562): running maximum starts at 0, strict '>': lowest symbol among the maxima, 0 without
    a positive entry."""
    k = int(np.argmax(P))
    return k + 1 if P[k] > 0 else 0


def decode(od, gf_mul, L_ch, layer_of, max_iter, fixed_iters=0):
    """One frame.  od: pyoracle.Decoder(method EMS, mode CANONICAL) on the code (its check() is the per-check update); gf_mul the
    field's multiplication table [q][q]; L_ch [N][q-1]; layer_of [M].
    Returns out [N], converged, iters, post [N][q-1], c2v [E][q-1] (variable-major edge order, as nbl_read_state returns it)."""
    g = Graph(od.code)
    w = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    order = [m for l in range(int(max(layer_of)) + 1) for m in range(g.M) if layer_of[m] == l]
    assert sorted(order) == list(range(g.M))
    c2v = np.zeros((g.E, w))                             # check-major
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
            dec[n] = _decide(P)
        if not frozen:
            out = dec.copy()
        ok = True
        for m in range(g.M):
            s = 0
            for ce in range(g.coff[m], g.coff[m + 1]):
                s ^= int(gf_mul[g.c_h[ce], dec[g.c_var[ce]]])
            ok = ok and s == 0
        if ok and not frozen:
            frozen, iters = 1, it
            if not fixed_iters:
                break
        for m in order:
            vin = np.zeros((g.dc[m], w))
            for k in range(g.dc[m]):
                ce = g.coff[m] + k
                n = g.c_var[ce]
                P = L_ch[n].copy()
                for e in range(g.voff[n], g.voff[n + 1]):
                    P = P + c2v[g.v_slot[e]]             # the CURRENT values
                vin[k] = P - c2v[ce]
            c2v[g.coff[m]:g.coff[m + 1]] = od.check(m, vin)
    c2v_vm = np.zeros_like(c2v)
    c2v_vm[g.c2e] = c2v
    return out, frozen, iters, post.copy(), c2v_vm


def decode_batch(od, gf_mul, L, layer_of, max_iter, fixed_iters=0):
    return [decode(od, gf_mul, L[b], layer_of, max_iter, fixed_iters) for b in range(L.shape[0])]
