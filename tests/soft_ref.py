"""Bit-LLR input and soft output of include/nbldpc.h (nbl_decode_batch_bits, nbl_soft_output) restated in numpy -- TEST INFRASTRUCTURE
ONLY, for tests/test_soft.py (CPU) and tests/test_gpu_soft.py (HIP kernels).  Written as the header's formulas read, one Python loop per
order the header fixes (bits ascending, a variable's edges in its edge order, symbols ascending); frames are the only vectorised axis.

  bits_to_lch(lam, p)                  [..][N p] -> [..][N][q-1]: the RX_LLR_BIT -> RX_LLR_SYM loop (Comm.cpp:362-372), from 0.0
  posterior(L_ch, c2v_vm, graph)       P[n] = L_ch[n] + c2v of n's edges in n's edge order; c2v_vm [E][q-1] variable-major, as
                                       nbl_read_state and the oracle's state() return it; graph: layered_ref.Graph (or anything with
                                       N and voff)
  bit_marginals(P, p, metric, dtype)   [..][N][q-1] -> [..][N p]; dtype float64 or numpy.longdouble
  marginal_scale(P)                    max(1, max |P[n]|) per variable: what the log-sum tolerance is relative to
"""
import numpy as np

LOGSUM, MAXLOG = 0, 1

# Log-sum.  RESTATEMENT_LOGSUM_ERR is the worst error of the float64 restatement against the numpy.longdouble one, relative to
# max(1, max |P[n]|) of the variable, measured on the inputs of tests/test_gpu_soft.py (every posterior of its decoder grid; asserted in
# tests/test_soft.py on the frames of that grid a CPU can form: the channel vectors of every case and the oracle's posteriors of the
# EMS / T-EMS cases): 4.67 units of 2^-53, set by a GF(8) variable of the `all` degree profile (the shipped codes stay at or under 3.02).  The GPU is held to four times
# that, with the floor tests/demod_general.py uses (2^-49): the factor covers a device exp / log of 1-2 ulp where libm's are correctly
# rounded in practice, and a tree reduction of up to 128 terms where the definition sums in sequence.  The factor and its reason are
# that file's.  Worst error the MI355X showed on the same inputs: see GPU_LOGSUM_ERR.  DESIGN.md section 5h records all three.
RESTATEMENT_LOGSUM_ERR = 5.19e-16
LOGSUM_FLOOR = 2.0 ** -49
LOGSUM_TOL = max(4 * RESTATEMENT_LOGSUM_ERR, LOGSUM_FLOOR)
GPU_LOGSUM_ERR = 3.27e-16   # 2.95 units of 2^-53 (BDS576.288 GF(64), log-QSPA): inside the restatement's own error


def bits_to_lch(lam, p):
    """L_ch[..][n][a-1] = 0.0 + lam[n p + j0] + lam[n p + j1] ... over the set bits j of a, ascending"""
    lam = np.asarray(lam)
    q = 1 << p
    N = lam.shape[-1] // p
    assert lam.shape[-1] == N * p
    bit = lam.reshape(lam.shape[:-1] + (N, p))
    out = np.zeros(lam.shape[:-1] + (N, q - 1), dtype=lam.dtype)
    for a in range(1, q):
        s = np.zeros(lam.shape[:-1] + (N,), dtype=lam.dtype)
        for j in range(p):
            if (a >> j) & 1:
                s = s + bit[..., j]
        out[..., a - 1] = s
    return out


def posterior(L_ch, c2v_vm, graph):
    """AddLLRVector in the variable's edge order (NBLDPC.cpp:678-685): [N][q-1]"""
    L_ch, c2v_vm = np.asarray(L_ch), np.asarray(c2v_vm)
    P = np.array(L_ch, copy=True)
    for n in range(graph.N):
        for e in range(int(graph.voff[n]), int(graph.voff[n + 1])):
            P[n] = P[n] + c2v_vm[e]
    return P


def marginal_scale(P):
    """max(1, max |P[n]|): [..][N]"""
    return np.maximum(1.0, np.max(np.abs(np.asarray(P, dtype=np.float64)), axis=-1))


def bit_marginals(P, p, metric, dtype=np.float64):
    """P [..][N][q-1] (a = 1 .. q-1; a = 0 has the value 0.0) -> bit LLRs [..][N p], bit j of a symbol has value 2^j"""
    P = np.asarray(P, dtype=dtype)
    q = 1 << p
    assert P.shape[-1] == q - 1
    full = np.concatenate([np.zeros(P.shape[:-1] + (1,), dtype=dtype), P], axis=-1)   # slot a
    out = np.zeros(P.shape[:-1] + (p,), dtype=dtype)
    for j in range(p):
        val = []
        for want in (1, 0):
            S = [a for a in range(q) if ((a >> j) & 1) == want]
            M = full[..., S[0]]
            for a in S[1:]:
                M = np.maximum(M, full[..., a])
            if metric == MAXLOG:
                val.append(M)
            else:
                total = np.zeros(P.shape[:-1], dtype=dtype)
                for a in S:                                                          # ascending a
                    total = total + np.exp(full[..., a] - M)
                val.append(M + np.log(total))
        out[..., j] = (val[0] - val[1]) + dtype(0.0)                                 # (a zero difference is +0.0)
    return out.reshape(P.shape[:-2] + (P.shape[-2] * p,))


def bits_equal(a, b):
    """bit patterns, not values: a -0.0 against a +0.0 is a difference"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def logsum_error(got, want, P):
    """worst |got - want| relative to max(1, max |P[n]|) of the variable; got / want [..][N p], P [..][N][q-1]"""
    scale = marginal_scale(P)
    p = np.asarray(got).shape[-1] // scale.shape[-1]
    d = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(want, dtype=np.longdouble))
    return float(np.max(d.reshape(scale.shape + (p,)) / scale[..., None]))
