"""The dense generator of the host layer (hostlib.generator = CNBLDPC::Generator, what nbl_set_transmitter is given) and the PN
helper of the C ABI, without a GPU.  Expected values: the parity checks of the shipped code files, the host encoder (pinned to the
compiled reference by test_host_frontend.py), the compiled reference's recorded code words (tests/golden) and the PN register
clocked literally."""
import numpy as np
import pytest

from conftest import load_golden
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib

CODES = sorted(df.codes())
SETS = ["cfg1_bp_gf16", "cfg2_ems_u128", "cfg3_ems_u512", "ems_nc2_shaped", "cfg4_tems_bds", "cfg5_bp_c512"]


def _tables(q):
    mul, inv = df.gf_tables(q)
    return np.array(mul, dtype=np.int64), np.array(inv, dtype=np.int64)


def _apply(gen, msgs, mul):
    """code [B][N] = gen [N][K] * msg over GF(q) (addition is XOR)"""
    out = np.zeros((msgs.shape[0], gen.shape[0]), dtype=np.int64)
    for k in range(gen.shape[1]):
        out ^= mul[gen[:, k][None, :], msgs[:, k][:, None]]
    return out


def _eliminate(A, mul, inv):
    """reduced row echelon form of A over GF(q): (R, pivot columns)"""
    R = A.astype(np.int64).copy()
    piv, r = [], 0
    for c in range(R.shape[1]):
        rows = np.nonzero(R[r:, c])[0]
        if rows.size == 0:
            continue
        R[[r, r + rows[0]]] = R[[r + rows[0], r]]
        R[r] = mul[inv[R[r, c]], R[r]]
        for i in np.nonzero(R[:, c])[0]:
            if i != r:
                R[i] ^= mul[R[i, c], R[r]]
        piv.append(c)
        r += 1
        if r == R.shape[0]:
            break
    return R, piv


def _generator(tmp_path, code_name):
    c = df.codes()[code_name]
    q = c["q"]
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=q, code=code_name, method=2, ems_nm=min(q, 16), constellation="BPSK", random_msg=1), code_name, "BPSK")
    return c, hostlib.generator(str(tmp_path), c["N"], c["N"] - c["M"]).astype(np.int64)


@pytest.mark.parametrize("code_name", CODES)
def test_generator_satisfies_every_check_and_equals_the_encoder(tmp_path, code_name):
    c, gen = _generator(tmp_path, code_name)
    N, M, q = c["N"], c["M"], c["q"]
    K = N - M
    mul, _ = _tables(q)
    assert gen.shape == (N, K) and gen.max() < q
    for m, row in enumerate(c["chk_rows"]):       # H gen = 0, column by column
        s = np.zeros(K, dtype=np.int64)
        for v, h in row:
            s ^= mul[h, gen[v - 1]]
        assert not s.any(), (code_name, m)
    rng = np.random.default_rng(11)
    msgs = np.concatenate([np.zeros((1, K), dtype=np.int64), np.eye(K, dtype=np.int64), rng.integers(0, q, (40, K))])
    assert np.array_equal(_apply(gen, msgs, mul), hostlib.encode(str(tmp_path), msgs, N))


@pytest.mark.parametrize("name", SETS)
def test_generator_reproduces_the_reference_code_words(tmp_path, name):
    g, meta = load_golden(name)
    c, gen = _generator(tmp_path, meta["code"])
    K, q = c["N"] - c["M"], c["q"]
    mul, inv = _tables(q)
    tx = g["tx_code"].astype(np.int64)
    R, piv = _eliminate(np.concatenate([gen[:K], np.eye(K, dtype=np.int64)], axis=1), mul, inv)
    if piv == list(range(K)):                     # rows 0 .. K-1 of gen are invertible: m = A^-1 tx[:K], then the whole word from it
        Ainv = R[:, K:]
        m = _apply(Ainv, tx[:, :K], mul)
        assert np.array_equal(_apply(gen, m, mul), tx), name
    else:                                         # they are not for this code: the word must still lie in the column space of gen
        print(f"{name}: rows 0..K-1 of the generator are singular, checking the column space instead")
        for row in tx:
            Rr, pv = _eliminate(np.concatenate([gen, row[:, None]], axis=1), mul, inv)
            assert K not in pv, name
    # what Err compares against is the head of the code word (Encode rewrites the message)
    assert np.array_equal(g["tx_msg"], tx[:, :K])


def _literal(state, clocks):
    """GenPN clocked literally (Comm.cpp:241-252): shift, then regPN[0] = regPN[10] ^ regPN[3]"""
    r = [(state >> i) & 1 for i in range(11)]
    for _ in range(clocks):
        r = [0] + r[:10]
        r[0] = r[10] ^ r[3]
    return sum(b << i for i, b in enumerate(r))


@pytest.mark.parametrize("state", [hostlib.pn_initial(0), hostlib.pn_initial(7), 1, 0x400, 0x7ff, 0])
def test_pn_advance_equals_literal_clocking(state):
    for clocks in (0, 1, 2046, 2047, 2048):
        want = _literal(state, clocks)
        assert hostlib.pn_clock(state, clocks) == want    # the host layer's GenPN is the literal register
        assert hostlib.pn_advance(state, clocks) == want, (state, clocks)
    assert hostlib.pn_advance(state, 10**9) == hostlib.pn_clock(state, 10**9)   # 10^9 literal calls of GenPN


def test_pn_initial_is_the_reference_register():
    init = [1, 0, 1, 0, 0, 0, 1, 1, 0, 0, 1]    # Comm.cpp:58-74
    s0 = sum(b << i for i, b in enumerate(init))
    assert hostlib.pn_initial(0) == s0
    for lane in (1, 2, 100, 5000):
        assert hostlib.pn_initial(lane) == _literal(s0, lane) == hostlib.pn_advance(s0, lane)
