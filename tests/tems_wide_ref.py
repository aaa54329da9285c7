"""The T-EMS check node as the kernels evaluate it (nbl_cn_tems_core.h, nbl_cn_tems_wide_core.h), restated in numpy with the path kept as
the dense digit tuple (q_0 .. q_d) and the rule for equal costs as a parameter -- TEST INFRASTRUCTURE ONLY.

It exists to show that an input discriminates: on LLRs whose sums are exact and tie often, tie="first" (the first path in enumeration
order, the reference's rule) must reproduce the oracle's check node bit for bit and tie="last" must not.  Nothing else is compared
with it; the reference of every GPU comparison is the oracle."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def shape_llr(y, factor, offset):
    if factor == 1.0 and offset == 0.0:
        return y if (y < 0.0 or y > 0.0) else 0.0
    if factor != 1.0:
        y = y / factor
    if y < -1 * offset:
        return y + offset
    if y > offset:
        return y - offset
    return 0.0


def check_node(vin, h, gf_mul, nr, nc, factor=1.0, offset=0.0, tie="first"):
    """vin [dc][q-1]: the incoming vectors of a check (symbol 0 implicit, 0.0); h [dc] its coefficients; gf_mul [q][q].
    Returns the outgoing vectors [dc][q-1]."""
    assert tie in ("first", "last")
    dc, q = vin.shape[0], vin.shape[1] + 1
    L = np.concatenate([np.zeros((dc, 1)), np.asarray(vin, dtype=np.float64)], axis=1)
    beta, dU = [], np.zeros((dc, q))
    for d in range(dc):
        best, arg = 0.0, 0
        for a in range(q):
            if L[d, a] > best:
                best, arg = L[d, a], a
        b = int(gf_mul[h[d], arg])
        beta.append(b)
        for a in range(q):
            dU[d, int(gf_mul[h[d], a]) ^ b] = best - L[d, a]
    syn = 0
    for b in beta:
        syn ^= b
    marks, ord01 = [], []
    for s in range(q):
        order = sorted(range(dc), key=lambda d: (dU[d, s], d))
        marks.append(set(order[:nr]))
        ord01.append((order[0], order[1]))

    def better(val, code, bv, bc):
        if val < bv:
            return True
        return val == bv and (code < bc if tie == "first" else code > bc)

    inf = float("inf")
    cost = [[0.0 if (l == 0 and s == 0) else inf for s in range(q)] for l in range(nc + 1)]
    path = [[() for s in range(q)] for l in range(nc + 1)]
    for d in range(dc):
        cand = [s for s in range(1, q) if d in marks[s]]
        ncost = [[cost[l][s] + 0.0 for s in range(q)] for l in range(nc + 1)]
        npath = [[path[l][s] + (0,) for s in range(q)] for l in range(nc + 1)]
        for l in range(1, nc + 1):
            for dev in cand:
                u = dU[d, dev]
                for s in range(q):
                    val, code = cost[l - 1][s ^ dev] + u, path[l - 1][s ^ dev] + (dev,)
                    if better(val, code, ncost[l][s], npath[l][s]):
                        ncost[l][s], npath[l][s] = val, code
        cost, path = ncost, npath
    dW, eta = [inf] * q, [None] * q
    for s in range(q):
        for l in range(nc + 1):
            if eta[s] is None or better(cost[l][s], path[l][s], dW[s], eta[s]):
                dW[s], eta[s] = cost[l][s], path[l][s]
    out = np.zeros((dc, q - 1))
    for d in range(dc):
        Lc = [DBL_MAX] * q
        for s in range(q):
            dev = eta[s][d]
            Lc[s ^ dev] = min(Lc[s ^ dev], dW[s] - dU[d, dev])
        for s in range(q):
            if Lc[s] == DBL_MAX:
                o0, o1 = ord01[s]
                Lc[s] = dU[o1, s] if d == o0 else dU[o0, s]
        bsyn = syn ^ beta[d]
        L0 = -1.0 * Lc[bsyn]
        for a in range(1, q):
            out[d, a - 1] = shape_llr(-1.0 * Lc[int(gf_mul[h[d], a]) ^ bsyn] - L0, factor, offset)
    return out
