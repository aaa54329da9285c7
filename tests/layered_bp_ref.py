"""The damped layered (check-serial) log-QSPA schedule of include/nbldpc.h (nbl_create_layered_bp), restated in numpy -- TEST
INFRASTRUCTURE ONLY.

It is tests/layered_tems_ref.py with two changes: the per-check update is the oracle's log-QSPA single-check entry point
(pyoracle.Decoder(method BP, mode CANONICAL).check: the FP64 restatement of NBLDPC.cpp:747-767 that flooding log-QSPA is pinned to by
tests/test_gpu_parity.py), and the blend of the reference's per-edge damping is 0.5 old + 0.5 new (NBLDPC.cpp:730-741).

log-QSPA is not reproduced bit for bit (the reference's log-sum-exp is 80-bit and sequential, the oracle's and the kernels' are FP64,
each in its own order), so a comparison of hard decisions is only meaningful where no decision hangs on the last bits.  decode()
therefore also returns the smallest gap between the two largest candidates of any DecideLLRVector call it makes (a-posteriori, raw and
stored v2c; the implicit 0 of symbol 0 is a candidate): the tests require it to be orders of magnitude above the 1e-9 the LLRs agree to.
"""
import numpy as np

from layered_ref import Graph, _decide, greedy_layers  # noqa: F401  (greedy_layers: re-exported for the tests)


def _gap(P):
    """distance between the two largest of (0, P[0], .., P[q-2]): how far DecideLLRVector(P) is from deciding otherwise"""
    top = np.partition(np.concatenate([[0.0], P]), -2)[-2:]
    return float(top[1] - top[0])


def decode(od, gf_mul, L_ch, layer_of, max_iter, fixed_iters=0, damp=True):
    """One frame.  od: pyoracle.Decoder(method BP, mode CANONICAL) on the code (its check() is the per-check update); gf_mul the
    field's multiplication table [q][q]; L_ch [N][q-1]; layer_of [M].  damp=False leaves the damping out (only to show that it
    matters).
    Returns out [N], converged, iters, post [N][q-1], c2v [E][q-1], v2c [E][q-1] (both in variable-major edge order, as nbl_read_state
    returns them), the number of edge visits and of blends taken, and the smallest decide gap (see above)."""
    g = Graph(od.code)
    w = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    order = [m for l in range(int(max(layer_of)) + 1) for m in range(g.M) if layer_of[m] == l]
    assert sorted(order) == list(range(g.M))
    c2v = np.zeros((g.E, w))                             # check-major
    v2c = L_ch[g.c_var].copy()                           # check-major: v2c[(m,k)] = L_ch[n] (NBLDPC.cpp:647-655)
    post = np.zeros((g.N, w))
    out = np.zeros(g.N, dtype=np.int32)
    frozen, iters = 0, max_iter
    visits = blends = 0
    gap = np.inf
    for it in range(1, max_iter + 1):
        dec = np.zeros(g.N, dtype=np.int32)
        for n in range(g.N):
            P = L_ch[n].copy()
            for e in range(g.voff[n], g.voff[n + 1]):
                P = P + c2v[g.v_slot[e]]
            post[n] = P
            dec[n] = _decide(P)
            gap = min(gap, _gap(P))
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
                raw = P - c2v[ce]
                old = v2c[ce]
                visits += 1
                gap = min(gap, _gap(raw), _gap(old))
                if damp and _decide(raw) != _decide(old):
                    raw = 0.5 * old + 0.5 * raw          # two rounded products, one rounded sum (no contraction in numpy)
                    blends += 1
                v2c[ce] = raw
                vin[k] = raw
            c2v[g.coff[m]:g.coff[m + 1]] = od.check(m, vin)
    c2v_vm, v2c_vm = np.zeros_like(c2v), np.zeros_like(v2c)
    c2v_vm[g.c2e] = c2v
    v2c_vm[g.c2e] = v2c
    return out, frozen, iters, post.copy(), c2v_vm, v2c_vm, visits, blends, gap


def decode_batch(od, gf_mul, L, layer_of, max_iter, fixed_iters=0, damp=True):
    return [decode(od, gf_mul, L[b], layer_of, max_iter, fixed_iters, damp) for b in range(L.shape[0])]
