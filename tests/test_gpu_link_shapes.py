"""The device link chain (transmitter, channel, demodulator, error count, plain encoder) on every shape of tests/link_shapes.py: fields
with p = 2, 3, 5, 7, sizes that are no multiple of any tile, encoders with column exchanges, CRC lengths at the edges, q-ary
modulation with punctured symbols, PN strides at and above the register's period.  Every expected value is the compiled reference's
(tests/golden/link_shape_*.npz, fer_anchors_link.json) or the host chain's, which tests/test_link_shapes.py pins to the compiled
reference bit for bit on the same shapes; none is the device code's own.  Every comparison is equality of integers or bit patterns."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_golden
import link_shapes as ls
from link_util import Link, prepare_spec_workdir
import nbldpc_amd as nb
from nbldpc_amd import hostlib

pytestmark = pytest.mark.gpu

ALL = sorted(ls.SHAPES)
ANCHORS = json.load(open(os.path.join(GOLD, "fer_anchors_link.json")))
EXCHANGE = ("exchange_msg", "exchange_msg_crc24", "exchange_chain")
ODD_FIELDS = ("one_word", "gf8_odd", "gf32_63", "gf128_crc24")   # p = 2, 3, 5, 7
KEYS = ("EbN0", "frames", "errFrame", "errSym", "errBit", "U_errFrame", "FER", "SER", "BER")


def fixture(name):
    """(arrays, Eb/N0, frames, lanes) of a shape's fixture; the shapes the compiled reference cannot run have none"""
    if name in ls.NO_REFERENCE:
        return None, 3.0, 3, 3
    g, meta = load_golden(f"link_shape_{name}")
    return g, meta["ebn0"], meta["frames"], meta["profile"]["parallel"]


def link(tmp_path, name, P, **kw):
    over = kw.pop("over", {})
    _, spec, info = ls.shape(name)
    ln = Link(tmp_path, ls.profile_of(name, P, **over), None, None, P, spec=spec, points=ls.points_of(name), poly=ls.poly_of(name), **kw)
    assert (ln.L, ln.punct, ln.K, ln.p, ln.order) == (info["L"], info["punct"], info["K"], info["p"], info["order"])
    return ln, info


@pytest.mark.parametrize("name", ALL)
def test_transmit_side(tmp_path, name):
    g, ebn0, frames, P = fixture(name)
    ln, info = link(tmp_path, name, P)
    tx, msg, _ = ln.check_chain(ebn0, frames, *((g["tx_code"], g["tx_msg"]) if g is not None else ()))
    assert tx.any() == (info["nb"] > 0)          # crc_len == K p: no PN bit, the all-zero word with random_msg = 1
    if info["punct"]:
        assert ln.L < ln.N * ln.p // (ln.order.bit_length() - 1) and (ln.src == -1).sum() == len(info["punct"]) * (ln.p if ln.order == 2 else 1)
    ln.dec.close()


@pytest.mark.parametrize("tag", sorted(ls.stride_cases()))
def test_transmit_side_at_lane_strides_around_the_period(tmp_path, tag):
    g, meta = load_golden(f"link_shape_stride_{tag}")
    P = meta["profile"]["parallel"]
    assert P == ls.stride_cases()[tag]
    ln, _ = link(tmp_path, ls.SMALLEST, P)
    tx, _, _ = ln.check_chain(meta["ebn0"], meta["frames"], g["tx_code"], g["tx_msg"])
    assert (len(np.unique(tx, axis=0)) == 2) == (P % ls.pn_period() == 0)   # whole periods: every lane's draw is constant
    ln.dec.close()


@pytest.mark.parametrize("name", ALL)
def test_demodulator(tmp_path, name):
    g, ebn0, frames, P = fixture(name)
    ln, info = link(tmp_path / "a", name, P, with_tx=False)
    Lh, _, _, sigma = hostlib.frontend(ln.dir, ebn0, frames, ln.N, ln.K, ln.q, P)
    L = g["L_ch"] if g is not None else Lh
    rx, _, _, sigma2 = hostlib.channel(ln.dir, ebn0, frames, ln.L, P)
    assert sigma == sigma2 and np.array_equal(L.view(np.uint64), Lh.view(np.uint64))
    if info["punct"]:   # the LLRs of a punctured symbol are zeros, every other symbol has none (real-valued samples)
        assert not L[:, info["punct"]].any() and np.delete(L, info["punct"], axis=1).all()
    a = ln.dec.decode_samples(rx, sigma)
    b = ln.dec.decode(L)
    for x, y, what in zip(a, b, ("out", "converged", "iters")):
        assert np.array_equal(x, y), what
    ln.dec.close()
    # the posteriors after one iteration, bit for bit
    one, _ = link(tmp_path / "b", name, P, with_tx=False, over=dict(max_iter=1))
    one.dec.record_state(True)
    B = rx.shape[0]
    one.dec.decode_samples(rx, sigma)
    post_a = [one.dec.read_state(k)[0] for k in range(B)]
    one.dec.decode(L)
    for k in range(B):
        assert np.array_equal(post_a[k].view(np.uint64), one.dec.read_state(k)[0].view(np.uint64)), k
    one.dec.close()


def crc_check(bits, crc_len):
    """CrcCheck(bits, n, crc_len, 1) literally: the division register with the type-1 polynomial of CRC-24, an all-zero word is no pass"""
    if crc_len == 0:
        return 1
    taps = {8: (0, 1, 3, 4, 7), 16: (0, 5, 12), 24: (0, 1, 5, 6, 23)}[crc_len]
    reg = [0] * crc_len
    for x in bits:
        fb = reg[crc_len - 1]
        reg = [0] + reg[:-1]
        if fb:
            for t in taps:
                reg[t] ^= 1
        reg[0] ^= int(x)
    return int(not any(reg) and any(bits))


def host_words(dirpath, gen, info, name, tx, msg):
    """The decoded words of the error-count test (ten lanes) and the host chain's counts of them, with the sanity assertions on the
    host's answer.  No GPU."""
    N, K, p, q, crc_len = info["N"], info["K"], info["p"], info["q"], info["crc_len"]
    systematic = np.array_equal(gen[:K], np.eye(K, dtype=gen.dtype))
    assert systematic == (not any(left < K for _, left in info["swaps"]))
    if name in EXCHANGE:
        assert not systematic     # Encode exchanges a message column: a CRC-valid message does not stay one
    assert np.array_equal(msg, tx[:, :K])                                 # the slot's message: as Encode leaves it
    rng = np.random.default_rng(5)
    words = tx.copy()
    pos = sorted({0, min(3, K - 1), K - 1})
    flips = [1, q - 1, 2][:len(pos)]
    words[1, pos] ^= np.array(flips)                                      # symbol errors in the message part
    words[2, K:] ^= rng.integers(1, q, N - K)                             # errors in the parity part only
    # another valid code word whose PN draw carries a valid CRC under the polynomial CrcCheck uses (type 1 for CRC-24)
    bits = hostlib.crc_encode(rng.integers(0, 2, K * p - crc_len), crc_len, 1)
    other = (bits.reshape(K, p) << np.arange(p)).sum(axis=1)
    words[3] = hostlib.encode(dirpath, other[None, :], N)[0]
    words[4] = 0                                                          # the all-zero word
    words[5] = rng.integers(0, q, N)
    words[6, min(1, K - 1)] ^= 1                                          # one bit
    # rows 0 and 7 - 9 stay what was sent: valid codewords of a PN draw with a valid (type 0) CRC
    want = hostlib.err_count(dirpath, msg, words)
    assert want[0][0] == 0 and want[0][1] == len(pos) and want[1][1] == sum(bin(f).count("1") for f in flips), want
    assert want[0][2] == 0 and want[1][2] == 0 and want[0][6] == 1 and want[1][6] == 1, want
    assert (want[0][[7, 8, 9]] == 0).all() and (want[0][4] > 0) == bool(msg[4].any()), want
    # crc_ok is CrcCheck of the first K decoded symbols, literally -- whatever that says of a word
    literal = [crc_check([(int(s) >> k) & 1 for s in w[:K] for k in range(p)], crc_len) for w in words]
    assert want[2].tolist() == literal, (want[2], literal)
    if info["nb"] > 0:
        assert want[0][3] > 0, want                                      # the second code word is another one
    if systematic and other.any():   # no exchange: its message is its CRC-carrying draw, whose CRC (of CrcCheck's polynomial) holds
        assert want[2][3] == 1, want
    if systematic and crc_len in (8, 16):   # sent words pass their own CRC (CRC-24 is generated with one polynomial and checked with another)
        assert want[2][[0, 7, 8, 9]].tolist() == [int(w[:K].any()) for w in words[[0, 7, 8, 9]]], want
    if name == "exchange_msg":
        # .. but not behind a column exchange: the message Err looks at is not the PN draw, and its CRC does not hold
        assert not want[2][[0, 7, 8, 9]].all() and not want[2][3], want
        assert not np.array_equal(words[3, :K], other)
    return words, want


@pytest.mark.parametrize("name", ALL)
def test_error_count_equals_the_host_chain(tmp_path, name):
    B = 10
    ln, info = link(tmp_path, name, B)
    tx, msg, rx, txi, state, sigma = ln.host_chain(8.0, 1)
    pn, st = ln.states(1, state[:B])[0]
    ln.dec.transmit_batch(0, pn, st, sigma)
    words, want = host_words(ln.dir, ln.gen, info, name, tx, msg)
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
    assert want[0].sum() > 0 or info["K"] <= 2      # (a message of one or two symbols may survive)
    for w, gt in zip(want, got):
        assert np.array_equal(w, gt)
    ln.dec.close()


def _encode(ln, B, seed):
    msgs = np.random.default_rng(seed).integers(0, ln.q, (B, ln.K))
    msgs[0] = 0
    msgs[-1] = ln.q - 1
    want = hostlib.encode(ln.dir, msgs, ln.N)
    cw, mo = ln.dec.encode_batch(msgs)
    assert np.array_equal(cw, want)
    assert np.array_equal(mo, want[:, :ln.K])
    return msgs, want


def test_encode_batch_chunks(tmp_path):
    """4096 messages per chunk: one short of it, exactly one chunk, one more, and two chunks and one more"""
    ln, _ = link(tmp_path, ls.SMALLEST, 2)
    for B in (4095, 4096, 4097, 8193):
        _encode(ln, B, B)
    ln.dec.close()


@pytest.mark.parametrize("name", sorted(set(EXCHANGE + ODD_FIELDS) - {ls.SMALLEST}) + [ls.SMALLEST])
def test_encode_batch_equals_the_host_encoder(tmp_path, name):
    ln, info = link(tmp_path, name, 2)
    msgs, want = _encode(ln, 1000, ln.q)
    if any(left < ln.K for _, left in info["swaps"]):
        assert not np.array_equal(want[:, :ln.K], msgs)      # msg_out is the first K code symbols, not the input
    with pytest.raises(nb.NblError):
        ln.dec.encode_batch(np.full((1, ln.K), ln.q))       # a symbol outside the field
    ln.dec.close()


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_fer_with_the_device_transmitter(tmp_path, monkeypatch, name):
    a = ANCHORS[name]
    assert sorted(ANCHORS) == sorted(ls.FER_SHAPES) and 0 < a["points"][0]["errFrame"] < a["points"][0]["frames"]
    monkeypatch.setenv("NBL_DEVICE_TX", "1")
    _, spec, _ = ls.shape(name)
    prepare_spec_workdir(str(tmp_path), a["profile"], spec, ls.points_of(name))
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == len(a["points"])
    for got, ref in zip(rows, a["points"]):
        for k in KEYS:
            assert got[k] == ref[k], (name, k, got, ref)


@pytest.mark.parametrize("name", ls.FIELD_SHAPES)
def test_generator_of_another_field_is_refused_by_the_default_table(tmp_path, name):
    """gen derived by the host encoder from the tables of the shape's modulus: nbl_set_transmitter's H * gen = 0 check passes on a
    decoder created with those tables and fails (NBL_ERR_ARG, on the host, before any kernel) on one created with the default
    tables -- the check multiplies with the decoder's own field."""
    from conftest import decoder_kwargs
    ln, info = link(tmp_path / "a", name, 2, with_tx=False)
    assert ln.gf is not None and not np.array_equal(ln.gf[0], ls.gf_np(ln.q)[0])
    ln.set_tx()                                                           # the shape's own field: accepted
    # the generator of the same graph under the default tables is another matrix
    prepare_spec_workdir(str(tmp_path / "b"), ls.profile_of(name, 2), ls.shape(name)[1], ls.points_of(name))
    assert not np.array_equal(hostlib.generator(str(tmp_path / "b"), ln.N, ln.K), ln.gen)
    other = nb.Decoder(ln.code, ln.prof["method"], ln.prof["max_iter"], poll_every=2, **decoder_kwargs(ln.prof))
    other.set_demodulator(ln.order, ln.L, ln.src, ln.points)
    with pytest.raises(nb.NblError) as e:
        other.set_transmitter(gen=ln.gen, crc_len=ln.prof["crc_len"], random_msg=1, parallel=2, punct=ln.punct, mod_order=ln.order, n_mod_sym=ln.L)
    assert e.value.status == -1 and "H * gen != 0" in str(e.value), e.value
    other.close()
    ln.dec.close()


def _refused(ln, status, **over):
    with pytest.raises(nb.NblError) as e:
        ln.set_tx(**over)
    assert e.value.status == status, e.value
    assert str(e.value).split(":", 1)[1].strip(), "empty nbl_last_error"
    return str(e.value)


def test_abi_refusals(tmp_path):
    ln, info = link(tmp_path / "a", "crc_fills_message", 4, with_tx=False)
    assert info["K"] * info["p"] == 8
    _refused(ln, -2, crc_len=16)                                          # crc_len above K p
    _refused(ln, -2, crc_len=24)
    ln.set_tx()                                                           # crc_len == K p is served
    ln.dec.close()
    for sub, name in (("b", "punct_ends"), ("c", "qary_gf8_punct")):
        ln, info = link(tmp_path / sub, name, 4, with_tx=False)
        pu = info["punct"]
        assert "ascending" in _refused(ln, -1, punct=pu[::-1])
        assert "ascending" in _refused(ln, -1, punct=[pu[0], pu[0]] + pu[1:])
        assert "below N" in _refused(ln, -1, punct=pu[:-1] + [ln.N])
        _refused(ln, -1, punct=[-1] + pu[1:])
        # one sample more than the kept bits carry (the demodulator is set for it, so that this is the only thing wrong)
        ln.dec.set_demodulator(ln.order, ln.L + 1, ln.src, ln.points)
        assert "more bits" in _refused(ln, -1, n_mod_sym=ln.L + 1)
        ln.dec.set_demodulator(ln.order, ln.L, ln.src, ln.points)
        ln.set_tx()
        ln.dec.close()
