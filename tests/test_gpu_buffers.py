"""The host layer's buffers on a real MI355X (nbldpc_amd/csrc/nbl_buf.h, nbl_decoder.h): one handle taken through batches of 2, 5
and 3 codewords by every family of entry points, so that every buffer is made, grown and then used below its size, and the
launchers' view of the workspace (NblWork) is rebuilt once.  A stale view or a stale buffer after a growth shows as an output that
differs from a fresh handle's, or as a byte count that depends on the path.

  code      divsalar.UNBLDPC.128.64.GF.16, EMS, three iterations
  set-up    the general demodulator (QPSK under GF(16), symbol 5 punctured, max-log), Rayleigh fading, a transmitter with CRC-8
  inputs    the batch of 2 and the batch of 3 are the first rows of the batch of 5: what the loop's buffers hold (survivors of a
            pass) can then only be largest at 5, and the byte count of the path equals that of batch 5 alone"""
import numpy as np
import pytest

import demod_general as dg
import nbldpc_amd as nb
from nbldpc_amd import hostlib

pytestmark = pytest.mark.gpu

NAME, SIGMA, BMAX, COHERENCE, CRC = "gf16_qpsk_aligned", 0.4, 5, 3, 8


def make(sh, gen):
    dec = nb.Decoder(dg.graph(NAME)[0], nb.METHOD_EMS, 3, ems_nm=8, ems_nc=2)
    dec.set_demodulator(sh["M"], sh["L"], sh["src"], sh["points"], metric=dg.MAXLOG)
    dec.set_fading("rayleigh", COHERENCE)
    dec.set_transmitter(gen, CRC, 1, BMAX, sh["punct"], sh["M"], sh["L"])
    return dec


def inputs(sh, K):
    rng = np.random.default_rng(2026)
    N, p, q, L = sh["N"], sh["p"], sh["q"], sh["L"]
    rx, txi = dg.samples(sh, BMAX, SIGMA, 7)
    return dict(lch=4.0 * rng.standard_normal((BMAX, N, q - 1)), bits=4.0 * rng.standard_normal((BMAX, N * p)), rx=rx,
                prior=rng.standard_normal((BMAX, N * p)), gain=rng.standard_normal((BMAX, L, 2)), txi=txi.astype(np.uint8),
                state=rng.integers(1, 30000, (BMAX, 3)).astype(np.uint32), msg=rng.integers(0, q, (BMAX, K)).astype(np.int32),
                pn=np.array([hostlib.pn_initial(i) for i in range(BMAX)], dtype=np.uint16))


def families(dec, x, B):
    """every family once at batch B -> {label: tuple of arrays}"""
    out = {}
    out["decode"] = dec.decode(x["lch"][:B])
    out["soft_output"] = dec.soft_output("maxlog")
    out["prior"] = dec.decode_samples(x["rx"][:B], SIGMA, prior=x["prior"][:B])
    out["csi"] = dec.decode_samples(x["rx"][:B], SIGMA, gain=x["gain"][:B])
    out["csi+prior"] = dec.decode_samples(x["rx"][:B], SIGMA, prior=x["prior"][:B], gain=x["gain"][:B])
    out["bits"] = dec.decode_bits(x["bits"][:B])
    out["soft_output after bits"] = dec.soft_output("logsum", extrinsic=True)
    out["idd"] = dec.decode_samples_idd(x["rx"][:B], SIGMA, 2, "maxlog")
    out["idd csi"] = dec.decode_samples_idd(x["rx"][:B], SIGMA, 2, "maxlog", gain=x["gain"][:B])
    out["noise"] = dec.decode_noise(x["txi"][:B], x["state"][:B], SIGMA)
    out["encode"] = dec.encode_batch(x["msg"][:B])
    for slot in (0, 1):
        dec.channel_batch(slot, x["txi"][:B], x["state"][:B], SIGMA)
        out[f"channel {slot}"] = (dec.read_slot_rx(slot, 0, B), dec.read_gains(slot, 0, B)) + dec.decode_resident(slot, SIGMA, B)
        out[f"channel {slot} idd"] = dec.decode_resident(slot, SIGMA, B, passes=2)
        dec.transmit_batch(slot, x["pn"][:B], x["state"][:B], SIGMA)
        out[f"transmit {slot}"] = dec.read_transmitted(slot, 0, B) + (dec.read_slot_rx(slot, 0, B), dec.read_gains(slot, 0, B)) + \
            dec.decode_resident(slot, SIGMA, B)
        out[f"errors {slot}"] = dec.count_errors(slot, B)
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_growth_leaves_no_stale_view_or_buffer(tmp_path):
    sh = dg.shape(NAME)
    N, K = sh["N"], sh["N"] - dg.graph(NAME)[0].M
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=sh["q"], method=2, max_iter=3, parallel=BMAX, nqam=2, random_msg=1, crc_len=CRC, seed=31,
                                                ems_nm=8, ems_nc=2), dg.U16, "BPSK")
    gen = hostlib.generator(str(tmp_path), N, K)
    x = inputs(sh, K)
    a = make(sh, gen)
    alone_bytes = None
    for B in (2, 5, 3):
        got = families(a, x, B)
        fresh = make(sh, gen)
        want = families(fresh, x, B)
        if B == BMAX:
            alone_bytes = fresh.workspace_bytes()
            print(f"passes used by the loop at batch {B}: {want['idd'][3].tolist()}, with gains {want['idd csi'][3].tolist()}; "
                  f"workspace_bytes {alone_bytes}")
            assert (want["idd"][3] == 2).any() and (want["idd csi"][3] == 2).any()   # the loop ran a second pass on survivors
        fresh.close()
        assert list(got) == list(want)
        for label in want:
            assert len(got[label]) == len(want[label]), (B, label)
            for i, (g, w) in enumerate(zip(got[label], want[label])):
                assert bits_equal(g, w), (B, label, i)
    assert a.workspace_bytes() == alone_bytes
    a.close()
    third = make(sh, gen)                                                     # and the device is still in order after both were closed
    third.close()
