"""The flooding log-QSPA schedule of the reference (NBLDPC.cpp:643-775), restated in numpy on top of the oracle's single-check entry point
-- TEST INFRASTRUCTURE ONLY.  It is to flooding what tests/layered_bp_ref.py is to the layered schedule: the per-check update is
pyoracle.Decoder(method BP, mode CANONICAL).check, the FP64 restatement of NBLDPC.cpp:747-767, which is generic in the check degree; the
loop around it is written out so that every DecideLLRVector call can report how far it is from deciding otherwise.
tests/test_bp_wide.py asserts that this loop gives what the oracle's own decoder gives, bit for bit.

Order inside an iteration, as in the reference: a-posteriori vectors and decisions, syndrome (early exit here), variable-node pass with
the 0.5 / 0.5 per-edge damping, check-node pass.  A frame that leaves at iteration i therefore keeps the v2c of iteration i - 1; the
kernels run the variable-node pass before the syndrome, which is why nbl_read_state does not promise that v2c (include/nbldpc.h)."""
import numpy as np

from layered_bp_ref import _gap
from layered_ref import Graph, _decide


def decode_flooding(od, gf_mul, L_ch, max_iter, fixed_iters=0):
    """One frame.  od: pyoracle.Decoder(method BP, mode CANONICAL) on the code; gf_mul [q][q]; L_ch [N][q-1].
    Returns out [N], converged, iters, post [N][q-1], c2v [E][q-1], v2c [E][q-1] (both in variable-major edge order, as nbl_read_state
    returns them) and the smallest decide gap (layered_bp_ref.py: a-posteriori, raw and stored v2c, the implicit 0 included)."""
    g = Graph(od.code)
    w = g.q - 1
    L_ch = np.ascontiguousarray(L_ch, dtype=np.float64)
    c2v = np.zeros((g.E, w))                             # check-major
    v2c = L_ch[g.c_var].copy()                           # check-major (NBLDPC.cpp:647-655)
    post = np.zeros((g.N, w))
    out = np.zeros(g.N, dtype=np.int32)
    frozen, iters, gap = 0, max_iter, np.inf
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
        for n in range(g.N):                             # :718-744
            for e in range(g.voff[n], g.voff[n + 1]):
                ce = g.v_slot[e]
                raw, old = post[n] - c2v[ce], v2c[ce]
                gap = min(gap, _gap(raw), _gap(old))
                if _decide(raw) != _decide(old):
                    raw = 0.5 * old + 0.5 * raw          # two rounded products, one rounded sum
                v2c[ce] = raw
        for m in range(g.M):                             # :747-767
            c2v[g.coff[m]:g.coff[m + 1]] = od.check(m, v2c[g.coff[m]:g.coff[m + 1]])
    c2v_vm, v2c_vm = np.zeros_like(c2v), np.zeros_like(v2c)
    c2v_vm[g.c2e] = c2v
    v2c_vm[g.c2e] = v2c
    return out, frozen, iters, post.copy(), c2v_vm, v2c_vm, gap
