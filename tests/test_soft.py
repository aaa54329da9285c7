"""Bit-LLR input and soft output without a GPU: the numpy restatement of include/nbldpc.h's definition (tests/soft_ref.py) against the
host chain, the reference-pinned oracle and brute force, and the restatement's own log-sum error on the inputs of tests/test_gpu_soft.py."""
import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib
import layered_ref as lr
import soft_ref as sr
import soft_cases as sc

U16, U256_16 = sc.U16, "divsalar.UNBLDPC.256.128.GF.16"


@pytest.mark.parametrize("code_name,punct_deg", [(U16, 0), (U256_16, 3)])
def test_bits_to_lch_reproduces_the_host_chains_bpsk_llrs(tmp_path, code_name, punct_deg):
    """hostlib.frontend frames of a BPSK profile and of a punctured one (every variable of degree 3): lam = -2 rx / sigma^2 with the
    punctured bits 0.0 (Comm.cpp:352-356), expanded by the restatement, against the frames' own L_ch, bit for bit"""
    c = df.codes()[code_name]
    N, K, q, P = c["N"], c["N"] - c["M"], c["q"], 4
    p = q.bit_length() - 1
    punct = [n for n, r in enumerate(c["var_rows"]) if len(r) == punct_deg]
    assert bool(punct) == bool(punct_deg)
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=q, code=code_name, method=2, max_iter=5, parallel=P, constellation="BPSK", random_msg=1,
                                                puncture_degree=punct_deg, ems_nm=8), code_name, "BPSK")
    Lsam = (N - len(punct)) * p
    L, _, _, sigma = hostlib.frontend(str(tmp_path), 3.0, 2, N, K, q, P)
    rx, _, _, sigma2 = hostlib.channel(str(tmp_path), 3.0, 2, Lsam, P)
    assert sigma == sigma2 and L.shape[0] == 2 * P
    lam = np.zeros((2 * P, N * p))
    keep = np.array([n not in punct for n in range(N) for _ in range(p)])
    lam[:, keep] = -2 * rx[:, :, 0] / (sigma * sigma)
    assert sr.bits_equal(sr.bits_to_lch(lam, p), L)
    if punct:
        assert not L[:, punct].any() and L[:, [n for n in range(N) if n not in punct]].all()


@pytest.mark.parametrize("method", ["ems", "tems"])
def test_posterior_of_the_oracles_c2v_is_the_oracles_l_post(oracle, method):
    """U128.64 GF(16), CANONICAL: on every frame that converged, L_ch + the oracle's c2v in the variable's edge order equals the
    oracle's L_post bit for bit -- the definition pinned to the reference-pinned oracle"""
    code, edges, _ = sc.graph(U16)
    L, _ = sc.frames(U16)
    ocode = oracle.Code(edges=edges)
    g = lr.Graph(ocode)
    kw = sc.EMS_KW[U16] if method == "ems" else sc.TEMS_KW
    od = oracle.Decoder(ocode, oracle.GF(16), oracle.EMS if method == "ems" else oracle.TEMS, sc.max_iter_of(method), oracle.CANONICAL, **kw)
    n = 0
    for b in range(L.shape[0]):
        r, out, it = od.decode(L[b])
        post, _, c2v = od.state()
        if r:
            P = sr.posterior(L[b], c2v, g)
            assert sr.bits_equal(P, post), (method, b, it)
            assert [lr._decide(P[v]) for v in range(code.N)] == out.tolist()
            n += 1
    assert 5 <= n < L.shape[0]


def _brute(Pn, p, metric):
    """one variable, scalar Python: the header's formulas with math.exp / math.log"""
    import math
    full = [0.0] + [float(x) for x in Pn]
    out = []
    for j in range(p):
        v = []
        for want in (1, 0):
            S = [full[a] for a in range(1 << p) if ((a >> j) & 1) == want]
            M = max(S)
            if metric == sr.MAXLOG:
                v.append(M)
            else:
                t = 0.0
                for x in S:
                    t = t + math.exp(x - M)
                v.append(M + math.log(t))
        out.append((v[0] - v[1]) + 0.0)
    return out


@pytest.mark.parametrize("q", [4, 256])
def test_marginals_equal_a_brute_force_loop(q):
    p = q.bit_length() - 1
    rng = np.random.default_rng(q)
    P = rng.normal(-2.0, 6.0, (12, q - 1))
    P[0] = -np.abs(P[0]) - 0.5                  # the maximum sits at a = 0 (value 0.0)
    P[1] = np.round(P[1])                       # ties
    P[2] = 0.0                                  # all equal, a = 0 included
    P[3, : q // 2] = -0.0
    for metric in (sr.MAXLOG, sr.LOGSUM):
        got = sr.bit_marginals(P[None], p, metric)[0].reshape(12, p)
        for n in range(12):
            want = _brute(P[n], p, metric)
            if metric == sr.MAXLOG:
                assert sr.bits_equal(got[n], np.array(want)), (q, n)
            else:
                assert np.allclose(got[n], want, rtol=0, atol=2.0 ** -45 * max(1.0, np.abs(P[n]).max())), (q, n)
    mx = sr.bit_marginals(P[None], p, sr.MAXLOG)[0].reshape(12, p)
    assert np.all(mx[0] < 0) and not mx[2].any() and not np.signbit(mx[2]).any()
    assert np.all(mx[0] == [P[0][[a - 1 for a in range(1, q) if (a >> j) & 1]].max() for j in range(p)])   # M0 = 0.0 there


def gpu_inputs():
    """every posterior vector of the GPU test's grid a CPU can form: the channel vectors of every graph (max_iter = 0, and what every
    other posterior is made from) and the oracle's posteriors of the EMS / T-EMS cells, early exit and fixed iterations"""
    for name in sc.FRAMES:
        code, _, _ = sc.graph(name)
        yield name, "lch", code, sc.frames(name)[0]
    for name, method, _ in sc.GRID:
        if method not in ("ems", "tems") or (name, method) == (sc.U256, "tems"):
            continue
        code, edges, _ = sc.graph(name)
        import pyoracle
        g = lr.Graph(pyoracle.Code(edges=edges))
        L = sc.frames(name)[0]
        for fixed in (0, 1):
            ref = sc.oracle_state(name, method, fixed)
            yield name, f"{method}-{fixed}", code, np.stack([sr.posterior(L[b], ref[b][3], g) for b in sorted(ref)])


def test_restatement_logsum_error_on_the_gpu_tests_inputs(oracle):
    """float64 against numpy.longdouble, relative to max(1, max |P[n]|): the figure the GPU's tolerance is four times of"""
    assert np.finfo(np.longdouble).nmant >= 63
    worst = {}
    for name, tag, code, P in gpu_inputs():
        p = code.q.bit_length() - 1
        e = sr.logsum_error(sr.bit_marginals(P, p, sr.LOGSUM), sr.bit_marginals(P, p, sr.LOGSUM, np.longdouble), P)
        worst[name] = max(worst.get(name, 0.0), e)
    print("restatement log-sum error in units of 2^-53:", {k: round(v * 2.0 ** 53, 2) for k, v in worst.items()})
    assert max(worst.values()) <= 1.25 * sr.RESTATEMENT_LOGSUM_ERR, worst


@pytest.mark.parametrize("name,method", sorted({(n, m) for n, m, _ in sc.GRID}))
def test_the_grids_frames_have_the_convergence_mix(oracle, name, method):
    """what tests/test_gpu_soft.py asserts again before it trusts a case: iteration 1, an even one, an odd one >= 3, two failures"""
    conv, its = sc.oracle_flags(name, method)
    assert sc.has_mix(conv, its), list(zip(conv.tolist(), its.tolist()))
