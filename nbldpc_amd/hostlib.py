"""ctypes access to nbldpc_amd/host/libnbldpc_host.so (the reference-compatible C++ host layer) for tests."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import datafiles

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(_HERE, "host", "libnbldpc_host.so")
SIM_BIN = os.path.join(_HERE, "host", "nbldpc_sim")
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise FileNotFoundError(f"{HOST_LIB} is missing: make -C nbldpc_amd/host")
        try:
            import torch  # noqa: F401  (same reason as in binding.load_library: one HIP runtime per process)
        except Exception:
            pass
        L = C.CDLL(HOST_LIB)
        L.nblh_frontend.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.nblh_channel.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.nblh_demod_general.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
        L.nblh_demod_general_prior.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
        L.nblh_channel_fading.argtypes = [C.c_char_p, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                          C.POINTER(C.c_ulonglong)]
        L.nblh_demod_csi.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                     C.c_int, C.c_int, C.c_void_p]
        L.nbl_rand_advance.argtypes = [C.c_void_p, C.c_uint64]  # (libnbldpc_hip.so's helper, pure host arithmetic)
        L.nbl_rand_advance.restype = None
        L.nblh_simulate.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int]
        L.nblh_encode.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]
        L.nblh_generator.argtypes = [C.c_char_p, C.c_void_p]
        L.nblh_err_count.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nblh_crc_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.nblh_pn_clock.argtypes = [C.c_int, C.c_ulonglong]
        L.nblh_pn_initial.argtypes = [C.c_int]
        L.nbl_pn_advance.argtypes = [C.c_void_p, C.c_uint64]  # (libnbldpc_hip.so's helper, reachable through this library's link)
        L.nbl_pn_advance.restype = None
        _lib = L
    return _lib


@contextlib.contextmanager
def workdir(path):
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def prepare_workdir(path, profile_kwargs, code_name, constellation_name):
    """Lay out SRC/, the code file, the constellation file and NBLDPC.Profile.txt like the reference's working directory."""
    from .profiles import profile_text
    kw = dict(profile_kwargs)
    datafiles.materialise(path, kw["gfq"], code_name, constellation_name)
    kw["code"] = code_name + ".txt"
    kw["constellation"] = constellation_name + ".txt"
    prof = os.path.join(path, "NBLDPC.Profile.txt")
    with open(prof, "w") as f:
        f.write(profile_text(**kw))
    return prof


def frontend(workdir_path, ebn0, frames, N, K, q, P):
    B = frames * P
    L = np.zeros((B, N, q - 1))
    tx = np.zeros((B, N), dtype=np.int32)
    msg = np.zeros((B, K), dtype=np.int32)
    sig = C.c_double(0)
    with workdir(workdir_path):
        rc = load().nblh_frontend(b"NBLDPC.Profile.txt", ebn0, frames, L.ctypes.data, tx.ctypes.data, msg.ctypes.data, C.byref(sig))
    if rc != 0:
        raise RuntimeError(f"nblh_frontend rc={rc}")
    return L, tx, msg, sig.value


def channel(workdir_path, ebn0, frames, L, P):
    """Host link chain up to the AWGN channel: (rx [B][L][2], tx_index [B][L] uint8, state [B][3] uint32, sigma), B = frames * P."""
    B = frames * P
    rx = np.zeros((B, L, 2))
    txi = np.zeros((B, L), dtype=np.uint8)
    state = np.zeros((B, 3), dtype=np.uint32)
    sig = C.c_double(0)
    with workdir(workdir_path):
        rc = load().nblh_channel(b"NBLDPC.Profile.txt", ebn0, frames, rx.ctypes.data, txi.ctypes.data, state.ctypes.data, C.byref(sig))
    if rc != L:
        raise RuntimeError(f"nblh_channel rc={rc} (expected MOD_SYM_LEN {L})")
    return rx, txi, state, sig.value


def demod_general(N, p, points, src, rx, sigma, metric):
    """CComm::DemodulateGeneral (the host layer's statement of nbl_set_demodulator_ex's general path) on rx [B][L][2] -> [B][N][2^p - 1].
    points [M][2], src [N p] label-bit index per code bit (-1 = not transmitted), metric 0 = log-sum, 1 = max-log.  No GPU."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    src = np.ascontiguousarray(src, dtype=np.int32)
    rx = np.ascontiguousarray(rx, dtype=np.float64)
    B, L = rx.shape[0], rx.shape[1]
    assert src.shape == (N * p,) and rx.shape == (B, L, 2) and points.shape[1] == 2
    out = np.zeros((B, N, (1 << p) - 1))
    rc = load().nblh_demod_general(N, p, points.shape[0], L, points.ctypes.data, src.ctypes.data, rx.ctypes.data, float(sigma), int(metric), B, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_demod_general rc={rc}")
    return out


def demod_general_prior(N, p, points, src, rx, sigma, metric, prior):
    """The prior-aware overload of CComm::DemodulateGeneral (include/nbldpc.h, nbl_decode_batch_samples_prior): prior [B][N p] bit LLRs
    ln P(1) / P(0) per code bit, or None (then it IS demod_general).  No GPU."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    src = np.ascontiguousarray(src, dtype=np.int32)
    rx = np.ascontiguousarray(rx, dtype=np.float64)
    B, L = rx.shape[0], rx.shape[1]
    assert src.shape == (N * p,) and rx.shape == (B, L, 2) and points.shape[1] == 2
    if prior is not None:
        prior = np.ascontiguousarray(prior, dtype=np.float64)
        assert prior.shape == (B, N * p), prior.shape
    out = np.zeros((B, N, (1 << p) - 1))
    rc = load().nblh_demod_general_prior(N, p, points.shape[0], L, points.ctypes.data, src.ctypes.data, rx.ctypes.data,
                                         None if prior is None else prior.ctypes.data, float(sigma), int(metric), B, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_demod_general_prior rc={rc}")
    return out


def channel_fading(workdir_path, ebn0, frames, L, P, coherence):
    """Host link chain up to the Rayleigh block-fading channel (CComm::Channel_Rayleigh, `coherence` samples per gain):
    (rx [B][L][2], gain [B][L][2], tx_index [B][L] uint8, state [B][3] uint32, sigma, draws), B = frames * P; draws = the uniform draws one
    frame moves a lane's generator.  No GPU."""
    B = frames * P
    rx = np.zeros((B, L, 2))
    gain = np.zeros((B, L, 2))
    txi = np.zeros((B, L), dtype=np.uint8)
    state = np.zeros((B, 3), dtype=np.uint32)
    sig = C.c_double(0)
    draws = C.c_ulonglong(0)
    with workdir(workdir_path):
        rc = load().nblh_channel_fading(b"NBLDPC.Profile.txt", ebn0, frames, int(coherence), rx.ctypes.data, gain.ctypes.data, txi.ctypes.data,
                                        state.ctypes.data, C.byref(sig), C.byref(draws))
    if rc != L:
        raise RuntimeError(f"nblh_channel_fading rc={rc} (expected MOD_SYM_LEN {L})")
    return rx, gain, txi, state, sig.value, int(draws.value)


def demod_csi(path, N, p, points, src, rx, gain, sigma, metric=0, prior=None):
    """The host layer's demodulators with per-sample gains (include/nbldpc.h, "demodulators with gains") on rx, gain [B][L][2] ->
    [B][N][2^p - 1].  path "general": CComm::DemodulateGeneral's gain overload (src [N p] label-bit indices, metric, prior [B][N p] or
    None; gain None = the gain-less function); "bpsk": src [N p] sample indices; "qary": src [N] sample indices.  No GPU."""
    code = {"general": 0, "bpsk": 1, "qary": 2}[path]
    points = np.ascontiguousarray(points, dtype=np.float64)
    src = np.ascontiguousarray(src, dtype=np.int32)
    rx = np.ascontiguousarray(rx, dtype=np.float64)
    B, L = rx.shape[0], rx.shape[1]
    assert rx.shape == (B, L, 2) and points.shape[1] == 2 and src.shape == ((N,) if code == 2 else (N * p,))
    if gain is not None:
        gain = np.ascontiguousarray(gain, dtype=np.float64)
        assert gain.shape == rx.shape, gain.shape
    if prior is not None:
        prior = np.ascontiguousarray(prior, dtype=np.float64)
        assert prior.shape == (B, N * p), prior.shape
    out = np.zeros((B, N, (1 << p) - 1))
    rc = load().nblh_demod_csi(code, N, p, points.shape[0], L, points.ctypes.data, src.ctypes.data, rx.ctypes.data,
                               None if gain is None else gain.ctypes.data, None if prior is None else prior.ctypes.data, float(sigma), int(metric), B,
                               out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_demod_csi rc={rc}")
    return out


def rand_advance(state, draws):
    """nbl_rand_advance of the C ABI (pure host arithmetic): the generator state [3] after `draws` uniform draws"""
    s = np.array(state, dtype=np.uint32)
    load().nbl_rand_advance(s.ctypes.data, int(draws))
    return s


def simulate(workdir_path, device=0, max_rows=32):
    rows = np.zeros((max_rows, 9))
    with workdir(workdir_path):
        n = load().nblh_simulate(b"NBLDPC.Profile.txt", device, rows.ctypes.data, max_rows)
    if n < 0:
        raise RuntimeError(f"nblh_simulate rc={n}")
    keys = ("EbN0", "errFrame", "errSym", "errBit", "U_errFrame", "frames", "BER", "SER", "FER")
    return [dict(zip(keys, rows[i])) for i in range(n)]


def encode(workdir_path, msgs, N):
    msgs = np.ascontiguousarray(msgs, dtype=np.int32)
    out = np.zeros((msgs.shape[0], N), dtype=np.int32)
    with workdir(workdir_path):
        rc = load().nblh_encode(b"NBLDPC.Profile.txt", msgs.ctypes.data, msgs.shape[0], out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_encode rc={rc}")
    return out


def generator(workdir_path, N, K):
    """The encoder of the profile's code as a dense map gen [N][K] uint16: code[n] = sum_k gen[n][k] * msg[k] over GF(q).  No GPU."""
    gen = np.zeros((N, K), dtype=np.uint16)
    with workdir(workdir_path):
        rc = load().nblh_generator(b"NBLDPC.Profile.txt", gen.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_generator rc={rc}")
    return gen


def err_count(workdir_path, tx_msg, decoded):
    """TakeDecoded + ErrCount of the host chain per frame: (err_sym, err_bit, crc_ok), int32 [B] each.  No GPU."""
    tx_msg = np.ascontiguousarray(tx_msg, dtype=np.int32)
    decoded = np.ascontiguousarray(decoded, dtype=np.int32)
    B = decoded.shape[0]
    es, eb, ok = (np.zeros(B, dtype=np.int32) for _ in range(3))
    with workdir(workdir_path):
        rc = load().nblh_err_count(b"NBLDPC.Profile.txt", tx_msg.ctypes.data, decoded.ctypes.data, B, es.ctypes.data, eb.ctypes.data, ok.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"nblh_err_count rc={rc}")
    return es, eb, ok


def crc_encode(bits, crc_len, type24=0):
    """CComm::CRCEncode: the bits followed by their crc_len parity bits (type24: which of the two CRC-24 polynomials)"""
    bits = np.ascontiguousarray(bits, dtype=np.int32)
    out = np.zeros(bits.size + crc_len, dtype=np.int32)
    load().nblh_crc_encode(bits.ctypes.data, bits.size, crc_len, type24, out.ctypes.data)
    return out


def pn_clock(state, clocks):
    """the PN register after `clocks` literal calls of CComm::GenPN"""
    return load().nblh_pn_clock(int(state), int(clocks))


def pn_initial(lane):
    """PN register of `lane` in front of its first frame of an Eb/N0 point"""
    return load().nblh_pn_initial(int(lane))


def pn_advance(state, clocks):
    """nbl_pn_advance of the C ABI (pure host arithmetic)"""
    s = np.array([state], dtype=np.uint16)
    load().nbl_pn_advance(s.ctypes.data, int(clocks))
    return int(s[0])
