"""The transmit side of the link chain and its error count on the GPU (nbl_set_transmitter, nbl_transmit_batch, nbl_count_errors,
nbl_encode_batch, nbl_read_transmitted; NBL_DEVICE_TX=1 in the harness).  Every expected value is the compiled reference's
(tests/golden) or the host chain's (hostlib.frontend / channel / encode / err_count, pinned to the compiled reference bit for bit by
tests/test_host_frontend.py), never the device code's own."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, decoder_kwargs, load_golden
from link_util import Link
import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
from nbldpc_amd import hostlib

pytestmark = pytest.mark.gpu

ANCHORS = json.load(open(os.path.join(GOLD, "fer_anchors.json")))
ANCHORS_BS = json.load(open(os.path.join(GOLD, "fer_anchors_bstems.json")))
ANCHORS_OSD = json.load(open(os.path.join(GOLD, "fer_anchors_osd.json")))
SETS = ["cfg1_bp_gf16", "cfg2_ems_u128", "cfg3_ems_u512", "ems_nc2_shaped", "cfg4_tems_bds", "cfg5_bp_c512"]


@pytest.mark.parametrize("name", SETS)
def test_chain_parity_with_the_compiled_reference(tmp_path, name):
    g, meta = load_golden(name)
    p = meta["profile"]
    ln = Link(tmp_path, p, meta["code"], meta["constellation"], p["parallel"])
    ln.check_chain(meta["ebn0"], meta["frames"], g["tx_code"], g["tx_msg"])
    ln.dec.close()


VARIANTS = {
    # anchor whose profile is taken, overrides, lanes, max_batch
    "punctured": ("ems_gf16_u256_punct3", {}, 24, 0),
    "crc16": ("ems_u128_crc16", {}, 24, 0),
    "crc24": ("ems_u128_crc24", {}, 24, 0),
    "crc0": ("ems_u128_crc16", dict(crc_len=0), 24, 0),
    "zero_msg": ("cfg2_ems_u128", dict(random_msg=0), 24, 0),
    "lanes_100": ("cfg2_ems_u128", {}, 100, 0),        # not a multiple of 64
    "lanes_1": ("cfg2_ems_u128", {}, 1, 0),
    "above_max_batch": ("cfg2_ems_u128", {}, 40, 8),
    "qam_random_msg": ("osd_tems_bds_o1_p4", dict(nqam=64, osd_order=-1), 12, 0),   # q-ary modulation of an encoded message
}


@pytest.mark.parametrize("case", sorted(VARIANTS))
def test_chain_parity_with_the_host_chain(tmp_path, case):
    anchor, over, P, max_batch = VARIANTS[case]
    a = dict(ANCHORS, **ANCHORS_OSD)[anchor]
    cons = "GRAY_64QAM" if over.get("nqam") == 64 else a["constellation"]
    ln = Link(tmp_path, dict(a["profile"], **over), a["code"], cons, P, max_batch=max_batch)
    if case == "punctured":
        assert ln.punct and ln.L < ln.N * ln.p
    tx, msg, _ = ln.check_chain(a["profile"].get("snr_begin", 2.0), 3)
    assert tx.any() == (case != "zero_msg")
    ln.dec.close()


@pytest.mark.parametrize("anchor,crc_len", [("ems_u128_crc24", 24), ("ems_u128_crc16", 16), ("cfg1_bp_gf16", 8), ("cfg2_ems_u128", 0)])
def test_error_count_equals_the_host_chain(tmp_path, anchor, crc_len):
    a = ANCHORS[anchor]
    B = 10
    ln = Link(tmp_path, dict(a["profile"], crc_len=crc_len), a["code"], a["constellation"], B)
    N, K, p, q = ln.N, ln.K, ln.p, ln.q
    assert np.array_equal(ln.gen[:K], np.eye(K, dtype=ln.gen.dtype))   # systematic head: a CRC-valid message stays one after Encode
    tx, msg, rx, txi, state, sigma = ln.host_chain(8.0, 1)
    pn, st = ln.states(1, state[:B])[0]
    ln.dec.transmit_batch(0, pn, st, sigma)
    rng = np.random.default_rng(5)
    words = tx.copy()
    words[1, [0, 3, K - 1]] ^= [1, q - 1, 2]                            # three symbol errors in the message part
    words[2, K:] ^= rng.integers(1, q, N - K)                            # errors in the parity part only
    # another valid code word whose message carries a valid CRC under the polynomial CrcCheck uses (type 1 for CRC-24)
    bits = hostlib.crc_encode(rng.integers(0, 2, K * p - crc_len), crc_len, 1)
    other = (bits.reshape(K, p) << np.arange(p)).sum(axis=1)
    words[3] = hostlib.encode(ln.dir, other[None, :], N)[0]
    words[4] = 0                                                         # the all-zero word
    words[5] = rng.integers(0, q, N)
    words[6, 1] ^= 1                                                     # one bit
    want = hostlib.err_count(ln.dir, msg, words)
    assert want[0][0] == 0 and want[0][1] == 3 and want[0][2] == 0 and want[0][3] > 0 and want[2][3] == 1 and want[2][4] == (crc_len == 0), want
    ln.dec.set_decoded(0, words)
    got = ln.dec.count_errors(0, B)
    for w, gt, what in zip(want, got, ("err_sym", "err_bit", "crc_ok")):
        assert np.array_equal(w, gt), (what, w, gt)
    # and behind a real decode with out_sym = NULL: only the counters cross
    none, conv, iters = ln.dec.decode_resident(0, sigma, B, want_out=False)
    assert none is None
    got = ln.dec.count_errors(0, B)
    out, conv2, iters2 = ln.dec.decode_resident(0, sigma, B)
    assert np.array_equal(conv, conv2) and np.array_equal(iters, iters2)
    want = hostlib.err_count(ln.dir, msg, out)
    for w, gt in zip(want, got):
        assert np.array_equal(w, gt)
    # heavily corrupted frames
    ln.dec.transmit_batch(1, pn, st, 3.0)
    out, _, _ = ln.dec.decode_resident(1, 3.0, B)
    got = ln.dec.count_errors(1, B)
    want = hostlib.err_count(ln.dir, msg, out)
    assert want[0].sum() > 0
    for w, gt in zip(want, got):
        assert np.array_equal(w, gt)
    ln.dec.close()


TIE_SENSITIVE = {"bp_gf16_u256_punct3"}   # tests/test_gpu_fer.py: log-QSPA with punctured variables, exact ties
KEYS = ("EbN0", "frames", "errFrame", "errSym", "errBit", "U_errFrame", "FER", "SER", "BER")
ALL_ANCHORS = dict(ANCHORS, **ANCHORS_BS, **ANCHORS_OSD)


def _simulate(tmp_path, a, device=0):
    hostlib.prepare_workdir(str(tmp_path), a["profile"], a["code"], a["constellation"])
    return hostlib.simulate(str(tmp_path), device=device)


def _check(name, rows, points):
    assert len(rows) == len(points)
    for got, ref in zip(rows, points):
        if name in TIE_SENSITIVE:   # the rule of tests/test_gpu_fer.py for this profile
            assert got["frames"] == ref["frames"], (name, got, ref)
            assert abs(got["errFrame"] - ref["errFrame"]) <= max(3, 0.1 * ref["errFrame"]), (name, "errFrame", got, ref)
            assert abs(got["errSym"] - ref["errSym"]) <= max(40, 0.15 * ref["errSym"]), (name, "errSym", got, ref)
            continue
        for k in KEYS:
            assert got[k] == ref[k], (name, k, got, ref)


def test_every_anchor_uses_a_constellation_the_device_transmitter_serves():
    assert {a["constellation"] for a in ALL_ANCHORS.values()} <= {"BPSK", "GRAY_64QAM", "GRAY_256QAM"}


@pytest.mark.parametrize("name", sorted(ALL_ANCHORS))
def test_fer_with_the_device_transmitter(tmp_path, monkeypatch, name):
    a = ALL_ANCHORS[name]
    monkeypatch.setenv("NBL_DEVICE_TX", "1")
    rows = _simulate(tmp_path, a)
    _check(name, rows, a["points"])
    if name in TIE_SENSITIVE:       # identical frames: count for count what the host transmitter gives on this build
        monkeypatch.setenv("NBL_DEVICE_TX", "0")
        off = _simulate(tmp_path, a)
        for got, ref in zip(rows, off):
            for k in KEYS:
                assert got[k] == ref[k], (name, k, got, ref)


def test_fer_with_the_device_transmitter_serial_driver(tmp_path, monkeypatch):
    monkeypatch.setenv("NBL_DEVICE_TX", "1")
    monkeypatch.setenv("NBL_PIPELINE", "0")
    a = ANCHORS["cfg2_ems_u128_p8"]
    _check("cfg2_ems_u128_p8", _simulate(tmp_path, a), a["points"])


def test_fer_with_the_device_transmitter_two_decoders(tmp_path, monkeypatch):
    monkeypatch.setenv("NBL_DEVICE_TX", "1")
    a = ANCHORS["cfg2_ems_u128_p8"]
    _check("cfg2_ems_u128_p8", _simulate(tmp_path, a, device=-2), a["points"])


def test_device_transmitter_needs_the_device_channel(tmp_path, monkeypatch):
    monkeypatch.setenv("NBL_DEVICE_TX", "1")
    monkeypatch.setenv("NBL_DEVICE_NOISE", "0")
    with pytest.raises(RuntimeError):
        _simulate(tmp_path, ANCHORS["cfg2_ems_u128_p8"])


def test_abi_refusals(tmp_path):
    a = ANCHORS["cfg2_ems_u128"]
    ln = Link(tmp_path, a["profile"], a["code"], a["constellation"], 4, with_tx=False)

    def refused(status, **over):
        with pytest.raises(nb.NblError) as e:
            ln.set_tx(**over)
        assert e.value.status == status, e.value
        assert str(e.value).split(":", 1)[1].strip(), "empty nbl_last_error"

    bad = ln.gen.copy()
    bad[ln.N - 1, 2] ^= 1
    refused(-1, gen=bad)                                   # H gen != 0
    refused(-1, crc_len=12)
    refused(-1, mod_order=ln.q)                            # differs from the demodulator's
    refused(-1, n_mod_sym=ln.L - 1)
    # transmitter before demodulator
    fresh = nb.Decoder(ln.code, ln.prof["method"], 5, **decoder_kwargs(ln.prof))
    with pytest.raises(nb.NblError) as e:
        fresh.set_transmitter(ln.gen, 8, 1, 4, [], 2, ln.L)
    assert e.value.status == -1 and "demodulator" in str(e.value)
    fresh.close()
    # out_sym = NULL without a transmitter, counting on a slot with no decode
    ln.set_tx()
    tx, msg, rx, txi, state, sigma = ln.host_chain(2.0, 1)
    pn, st = ln.states(1, state[:4])[0]
    ln.dec.transmit_batch(0, pn, st, sigma)
    with pytest.raises(nb.NblError) as e:
        ln.dec.count_errors(0, 4)
    assert e.value.status == -1 and "decode" in str(e.value)
    ln.dec.decode_resident(0, sigma, 4, want_out=False)
    ln.dec.count_errors(0, 4)
    with pytest.raises(nb.NblError):
        ln.dec.count_errors(1, 4)                          # the other slot holds nothing
    ln.dec.close()


@pytest.mark.parametrize("code_name", ["divsalar.UNBLDPC.512.256.GF.16", "BDS.576.288.GF.64", "divsalar.UNBLDPC.512.256.GF.256"])
def test_encode_batch_equals_the_host_encoder(tmp_path, code_name):
    q = df.codes()[code_name]["q"]
    ln = Link(tmp_path, dict(gfq=q, method=2, ems_nm=8, ems_nc=2, nqam=2, max_iter=5), code_name, "BPSK", 2)
    msgs = np.random.default_rng(q).integers(0, q, (1000, ln.K))
    msgs[0] = 0
    want = hostlib.encode(ln.dir, msgs, ln.N)
    cw, mo = ln.dec.encode_batch(msgs)
    assert np.array_equal(cw, want)
    assert np.array_equal(mo, want[:, :ln.K])
    with pytest.raises(nb.NblError):
        ln.dec.encode_batch(np.full((1, ln.K), q))         # a symbol outside the field
    ln.dec.close()
