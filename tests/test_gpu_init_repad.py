"""The set-up pass of a decode call on a real MI355X (nbl_kernels.hip: init_rows_kernel for q >= 64, init_kernel's loop below; DESIGN.md
section 2): the API layout [B][N][q-1] re-padded to [B][N][q] with slot 0 = 0.0.

q in {4, 16} take the element-wise loop, q in {64, 256} the row-wise kernel (two rows per wave at q = 64, one row in two passes at
q = 256); N in {5, 16} and B in {1, 3, 17} give row counts (5, 15, 16, 48, 85, 272) that are below, equal to and no multiple of the
rows a wave (4 or 8) and a workgroup (16 or 32) carry.  Per (q, N): L_ch as the decoder holds it (nbl_debug_read_lch) equals the input
bit for bit -- negative zeros and a row of extreme finite values included -- under each of the three forms of the pass: fused EMS
(the row kernel also clears the flags), T-EMS (v2c = L_ch for the damping) and the general kernels (c2v cleared); message state
after one iteration against the canonical oracle, T-EMS's v2c included; and a samples-in decode, where the demodulator has filled
L_ch and the pass re-pads nothing."""
import ctypes as C

import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
from degree_util import degree_code, ring_code

pytestmark = pytest.mark.gpu

QS, NS, BS = (4, 16, 64, 256), (5, 16), (1, 3, 17)
EMS, TEMS = nb.METHOD_EMS, nb.METHOD_TEMS


def graph(q, N):
    """N = 16: the (2, 4) ring of 8 checks; N = 5: three checks of degree 4, variables of degree 2, 3, 2, 3, 2"""
    if N == 16:
        code = ring_code(q, 8, 4)
        ev = np.repeat(np.arange(code.N, dtype=np.int32), code.var_deg)
        edges = (code.N, code.M, code.q, ev, code.var_chk.copy(), code.var_h.copy())
    else:
        code, edges, _ = degree_code(q, 600 + q, (4,), (2, 3), 3)
    assert code.N == N
    return code, edges


def params(q, method):
    return dict(ems_nm=min(q, 6), ems_nc=2, ems_factor=1.1, ems_offset=0.1) if method == EMS else dict(tems_nr=2, tems_nc=3, tems_factor=1.0, tems_offset=0.0)


def frames(q, N, B, seed):
    """real-valued rows; negative zeros scattered through every codeword; the last row of the first, a middle and the last codeword
    holds the extremes of FP64 (largest and smallest normal, subnormals, both signs, both zeros)"""
    rng = np.random.default_rng([seed, q, N, B])
    L = rng.normal(-1.5, 3.0, (B, N, q - 1))
    L[rng.random(L.shape) < 0.1] = -0.0
    L[:, 0, 0] = -0.0
    ext = np.array([np.finfo(np.float64).max, -np.finfo(np.float64).max, np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny, 5e-324, -5e-324, 0.0, -0.0])
    for b in {0, B // 2, B - 1}:
        L[b, N - 1] = np.resize(ext, q - 1)
    assert np.isfinite(L).all() and np.signbit(L[L == 0.0]).any()
    return L


def _force_generic(dec, on):
    dec.lib.nbl_debug_force_generic.argtypes = [C.c_void_p, C.c_int32]
    assert dec.lib.nbl_debug_force_generic(dec.h, int(on)) == 0


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("q", QS)
def test_lch_equals_the_input_bit_for_bit(q, N):
    """max_iter = 0: the call is the set-up pass alone (no kernel computes on the extreme values)"""
    code, _ = graph(q, N)
    for form, (method, generic) in enumerate(((EMS, 0), (TEMS, 0), (EMS, 1))):
        dec = nb.Decoder(code, method, 0, **params(q, method))
        _force_generic(dec, generic)
        for B in BS:
            L = frames(q, N, B, form)
            out, conv, its = dec.decode(L)
            assert not conv.any() and not its.any()
            for b in (0, B // 2, B - 1):
                assert dec.read_lch(b).tobytes() == L[b].tobytes(), (q, N, B, form, b)
        dec.close()


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("q", QS)
def test_state_after_one_iteration(oracle, q, N):
    """EMS and T-EMS, one iteration with state recording: T-EMS damps against v2c = L_ch, which only the set-up pass has written"""
    code, edges = graph(q, N)
    B = 17
    L = np.random.default_rng([9, q, N]).normal(-1.5, 3.0, (B, N, q - 1))
    for method in (EMS, TEMS):
        kw = params(q, method)
        dec = nb.Decoder(code, method, 1, **kw)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        od = oracle.Decoder(oracle.Code(edges=edges), oracle.GF(q), method, 1, oracle.CANONICAL, **kw)
        for b in (0, B // 2, B - 1):
            r, o, it = od.decode(L[b])
            assert (conv[b], its[b]) == (r, it) and np.array_equal(out[b], o), (q, N, method, b)
            for x, y in zip(dec.read_state(b), od.state()):
                assert np.array_equal(x, y), (q, N, method, b)
        dec.close()


@pytest.mark.parametrize("q,N", [(16, 5), (256, 16)])
def test_samples_in(oracle, q, N):
    """nbl_decode_batch_samples: the demodulator fills L_ch, the set-up pass gets no input to re-pad"""
    code, edges = graph(q, N)
    nbits = N * (q.bit_length() - 1)
    points = np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])])
    rng = np.random.default_rng([11, q])
    B, sigma = 3, 0.5
    rx = np.zeros((B, nbits, 2))
    rx[:, :, 0] = points[0, 0] + sigma * rng.standard_normal((B, nbits))
    rx[:, :, 1] = sigma * rng.standard_normal((B, nbits))
    kw = params(q, EMS)
    dec = nb.Decoder(code, EMS, 2, **kw)
    dec.set_demodulator(2, nbits, np.arange(nbits), points)
    got = dec.decode_samples(rx, sigma)
    lch = np.stack([dec.read_lch(b) for b in range(B)])
    state = [dec.read_state(b, post=False, v2c=False)[2] for b in range(B)]
    host = dec.decode(lch)
    for x, y in zip(got, host):
        assert np.array_equal(x, y)
    od = oracle.Decoder(oracle.Code(edges=edges), oracle.GF(q), EMS, 2, oracle.CANONICAL, **kw)
    for b in range(B):
        r, o, it = od.decode(lch[b])
        assert (got[1][b], got[2][b]) == (r, it) and np.array_equal(got[0][b], o), b
        assert np.array_equal(state[b], od.state()[2]), b
        assert lch[b].any()
    dec.close()
