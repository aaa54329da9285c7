"""Ordered-statistics decoding on the GPU (nbldpc_amd/csrc/nbl_osd.hip): against the compiled reference's fixtures, against the CPU
checker tests/osd_check.cpp bit for bit at scale, and across batch shapes and entry points."""
import glob
import json
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from nbldpc_amd import datafiles as df
from conftest import GOLD, load_golden
from osd_util import build_checker, decide, flag0_sums, osd_kwargs, profile, run_checker

pytestmark = pytest.mark.gpu

# (the osd_shape_* fixtures of the synthetic shapes hold several orders per file: tests/test_gpu_osd_shapes.py runs them)
SETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "osd_*.npz")) if not os.path.basename(p).startswith("osd_shape_"))
U512_256 = "divsalar.UNBLDPC.512.256.GF.256"
BDS = "BDS.576.288.GF.64"
U512_16 = "divsalar.UNBLDPC.512.256.GF.16"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("osd"))


def _method_kwargs(p):
    m = p["method"]
    if m == 2:
        return dict(ems_nm=p["ems_nm"], ems_nc=p["ems_nc"], ems_factor=p["ems_factor"], ems_offset=p["ems_offset"])
    if m == 4:
        return dict(tems_nr=p["tems_nr"], tems_nc=p["tems_nc"], tems_factor=p["tems_factor"], tems_offset=p["tems_offset"])
    if m == 7:
        return dict(bs_nm=p["bs_nm"], bs_nc=p["bs_nc"], bs_factor=p["bs_factor"], bs_offset=p["bs_offset"])
    return {}


@pytest.mark.parametrize("name", SETS)
def test_fixture_outputs_equal_reference(name):
    g, meta = load_golden(name)
    p = profile(meta)
    code = nb.Code(meta["code"])
    for k, it in enumerate(g["iters"]):
        dec = nb.Decoder(code, p["method"], int(it), **_method_kwargs(p), **osd_kwargs(p))
        out, conv, iters = dec.decode(g["L_ch"])
        dec.close()
        assert np.array_equal(out, g["out"][k]), (name, int(it))
        assert np.array_equal(conv, g["ret"][k]), (name, int(it))
        if p["method"] == 6:
            assert not iters.any()
        else:
            # the reference's iteration count: max_iter for a frame that did not converge (OSD leaves it alone), the iteration of
            # the first zero syndrome otherwise -- the same as without OSD
            assert (iters[conv == 0] == it).all() and ((iters[conv == 1] >= 1) & (iters[conv == 1] <= it)).all(), (name, int(it))
            off = nb.Decoder(code, p["method"], int(it), **_method_kwargs(p))
            _, o_conv, o_iters = off.decode(g["L_ch"])
            off.close()
            assert np.array_equal(conv, o_conv) and np.array_equal(iters, o_iters), (name, int(it))


def _frames(tmp_path, code_name, B, ebn0, seed, constellation="BPSK"):
    from nbldpc_amd import hostlib
    c = df.codes()[code_name]
    extra = dict(nqam=64, random_msg=0) if constellation != "BPSK" else dict(random_msg=1)
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=c["q"], code=code_name, method=2, max_iter=5, parallel=B, constellation=constellation,
                                                seed=seed, **extra), code_name, constellation)
    L, _, _, _ = hostlib.frontend(str(tmp_path), ebn0, 1, c["N"], c["N"] - c["M"], c["q"], B)
    return L


# (label, code, constellation, method kwargs, B, EbN0, iterations, order, crc_len, crc_rows)
SCALE = [
    ("cfg3_ems_o0", U512_256, "BPSK", dict(method=2, ems_nm=32, ems_nc=3), 256, 1.0, 2, 0, 8, 0),
    ("cfg3_ems_o1_crc8", U512_256, "BPSK", dict(method=2, ems_nm=32, ems_nc=3), 256, 1.0, 2, 1, 8, 8),
    ("cfg3_ems_o2_crc24", U512_256, "BPSK", dict(method=2, ems_nm=32, ems_nc=3), 64, 1.0, 2, 2, 24, 24),
    ("cfg4_tems_o2", BDS, "GRAY_64QAM", dict(method=4, tems_nr=2, tems_nc=3), 64, 3.0, 2, 2, 8, 0),
    ("gf16_generic_bp_o1_crc8", U512_16, "BPSK", dict(method=1), 128, 1.0, 2, 1, 8, 8),
    ("cfg3_ems_o3", U512_256, "BPSK", dict(method=2, ems_nm=32, ems_nc=3), 3, 0.5, 1, 3, 8, 0),
]


@pytest.mark.parametrize("label,code_name,cons,mkw,B,ebn0,iters,order,crc_len,crc_rows", SCALE)
def test_flag1_at_scale_vs_checker(tmp_path, checker, label, code_name, cons, mkw, B, ebn0, iters, order, crc_len, crc_rows):
    L = _frames(tmp_path, code_name, B, ebn0, 97, cons)
    code = nb.Code(code_name)
    mkw = dict(mkw)
    method = mkw.pop("method")
    dec = nb.Decoder(code, method, iters, **mkw, osd_order=order, osd_flag=1, crc_len=crc_len, crc_rows=crc_rows)
    out, conv, its = dec.decode(L)
    dec.close()
    off = nb.Decoder(code, method, iters, **mkw)
    o_out, o_conv, o_its = off.decode(L)
    off.close()
    assert np.array_equal(conv, o_conv) and np.array_equal(its, o_its), label
    assert np.array_equal(out[conv == 1], o_out[conv == 1]), label
    bad = np.flatnonzero(conv == 0)
    assert len(bad) > 0, label
    c_out = run_checker(checker, code, L[bad], order, 1, crc_len, crc_rows)
    assert np.array_equal(out[bad], c_out), (label, [int(b) for b in bad if not np.array_equal(out[b], c_out[list(bad).index(b)])][:8])


def test_method6_at_scale_vs_checker(tmp_path, checker):
    code_name = U512_256
    L = _frames(tmp_path, code_name, 128, 1.5, 5)
    code = nb.Code(code_name)
    dec = nb.Decoder(code, nb.METHOD_OSD, 10, osd_order=1, crc_len=16, crc_rows=16)
    out, conv, its = dec.decode(L)
    dec.close()
    assert not conv.any() and not its.any()
    assert np.array_equal(out, run_checker(checker, code, L, 1, 1, 16, 16))


@pytest.mark.parametrize("code_name,mkw", [(U512_256, dict(method=2, ems_nm=32, ems_nc=3)), (U512_16, dict(method=4, tems_nr=2, tems_nc=3))])
def test_flag0_sums_and_outputs(tmp_path, checker, code_name, mkw):
    """S pinned bit for bit against sum_t factor^(T-t) post_t rebuilt from read_state of decodes with max_iter = 1..T; the GPU's OSD
    against the checker fed with the GPU's S and the decisions of an OSD-off decode."""
    B, T, factor = 32, 3, 0.75
    L = _frames(tmp_path, code_name, B, 1.0, 11)
    code = nb.Code(code_name)
    mkw = dict(mkw)
    method = mkw.pop("method")
    posts = {}
    for t in range(1, T + 1):
        d = nb.Decoder(code, method, t, **mkw)
        d.record_state(True)
        d.decode(L)
        posts[t] = [d.read_state(b)[0] for b in range(B)]
        d.close()
    off = nb.Decoder(code, method, T, **mkw)
    o_out, o_conv, _ = off.decode(L)
    off.close()
    dec = nb.Decoder(code, method, T, **mkw, osd_order=1, osd_flag=0, osd_factor=factor)
    out, conv, _ = dec.decode(L)
    p = code.q.bit_length() - 1
    bad = np.flatnonzero(conv == 0)
    assert len(bad) > 0 and np.array_equal(conv, o_conv)
    S = np.zeros((len(bad), code.N * p))
    for j, b in enumerate(bad):
        S[j] = dec.debug_osd_sums(int(b)).reshape(-1)
        assert np.array_equal(S[j], flag0_sums([posts[t][b] for t in range(1, T + 1)], factor)), b
        assert np.array_equal(o_out[b], decide(posts[T][b])), b
    dec.close()
    c_out = run_checker(checker, code, L[bad], 1, 0, 8, 0, S=S, base=o_out[bad])
    assert np.array_equal(out[bad], c_out)
    assert np.array_equal(out[conv == 1], o_out[conv == 1])


def test_order_minus_one_is_create_ex():
    g, meta = load_golden("cfg2_ems_u128")
    code = nb.Code(meta["code"])
    L = g["L_ch"]
    a = nb.Decoder(code, nb.METHOD_EMS, 5, ems_nm=16, ems_nc=3)
    b = nb.Decoder(code, nb.METHOD_EMS, 5, ems_nm=16, ems_nc=3, osd_order=-1, osd_flag=0, osd_factor=0.5)
    for x, y in zip(a.decode(L), b.decode(L)):
        assert np.array_equal(x, y)
    a.profiling(True)
    b.profiling(True)
    a.decode(L)
    b.decode(L)
    assert a.last_timing()[1] == b.last_timing()[1]
    a.close()
    b.close()


def test_batch_shapes_and_entry_points():
    """B = 1, 7, 300 (> max_batch), polling against fixed iterations, and the device-pointer entry point: every codeword alike."""
    import torch
    g, meta = load_golden("osd_ems_gf16_o2")
    p = profile(meta)
    code = nb.Code(meta["code"])
    base = g["L_ch"]
    L = np.concatenate([base * (1.0 + 0.01 * k) for k in range(300 // base.shape[0] + 1)])[:300]
    kw = dict(**_method_kwargs(p), **osd_kwargs(p))
    ref = nb.Decoder(code, 2, 5, **kw, max_batch=64)
    r_out, r_conv, r_its = ref.decode(L)
    assert 0 < r_conv.sum() < len(L)
    for B in (1, 7, 300):
        got = ref.decode(L[:B])
        for a, r in zip(got, (r_out, r_conv, r_its)):
            assert np.array_equal(a, r[:B]), B
    for extra in (dict(poll_every=1), dict(fixed_iters=1)):
        d = nb.Decoder(code, 2, 5, **kw, **extra)
        out, conv, its = d.decode(L)
        assert np.array_equal(conv, r_conv) and np.array_equal(out, r_out), extra
        if not extra.get("fixed_iters"):
            assert np.array_equal(its, r_its)
        d.close()
    B = 64
    dL = torch.from_numpy(np.ascontiguousarray(L[:B])).cuda()
    out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    ref.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, r in zip((out, conv, its), (r_out, r_conv, r_its)):
        assert np.array_equal(a.cpu().numpy(), r[:B])
    ref.close()


ANCHORS = json.load(open(os.path.join(GOLD, "fer_anchors_osd.json")))


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_fer_matches_reference(tmp_path, name):
    """nbldpc_sim's main loop (hostlib.simulate) with OSD profiles: every count equals the compiled reference's."""
    from nbldpc_amd import hostlib
    a = ANCHORS[name]
    hostlib.prepare_workdir(str(tmp_path), a["profile"], a["code"], a["constellation"])
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == len(a["points"])
    for got, ref in zip(rows, a["points"]):
        for k in ("EbN0", "frames", "errFrame", "errSym", "errBit", "U_errFrame", "FER", "SER", "BER"):
            assert got[k] == ref[k], (name, k, got, ref)


def test_sim_binary_prints_osd_banner(tmp_path):
    import subprocess
    from nbldpc_amd import hostlib
    a = ANCHORS["osd_m6_gf256_o2_p8"]
    hostlib.prepare_workdir(str(tmp_path), dict(a["profile"], min_sim_cycle=16, snr_begin=3.0, snr_stop=3.0), a["code"], a["constellation"])
    out = subprocess.run([hostlib.SIM_BIN], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "Algorithm: OSD" in out.stdout and "OSD_order: 2" in out.stdout


@pytest.mark.parametrize("flag", [1, 0])
def test_samples_noise_and_resident_entry_points_equal_host_decode(tmp_path, flag):
    """nbl_decode_batch_samples, nbl_decode_batch_noise and nbl_channel_batch + nbl_decode_batch_resident give what the host entry
    point gives on the LLRs the device formed (read back with nbl_debug_read_lch)."""
    from nbldpc_amd import hostlib
    code_name, P, sigma_ebn0 = "divsalar.UNBLDPC.128.64.GF.256", 256, 1.0
    c = df.codes()[code_name]
    hostlib.prepare_workdir(str(tmp_path), dict(gfq=256, code=code_name, method=2, max_iter=3, parallel=P, constellation="BPSK",
                                                random_msg=1, seed=29), code_name, "BPSK")
    L = c["N"] * 8
    rx, txi, state, sigma = hostlib.channel(str(tmp_path), sigma_ebn0, 1, L, P)
    points = np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])])
    code = nb.Code(code_name)
    dec = nb.Decoder(code, nb.METHOD_EMS, 3, ems_nm=16, ems_nc=3, osd_order=1, osd_flag=flag, osd_factor=0.5, crc_len=8, crc_rows=8)
    dec.set_demodulator(2, L, np.arange(L), points)
    got = {"samples": dec.decode_samples(rx, sigma)}
    lch = np.stack([dec.read_lch(b) for b in range(P)])
    got["noise"] = dec.decode_noise(txi, state, sigma)
    dec.channel_batch(0, txi, state, sigma)
    got["resident"] = dec.decode_resident(0, sigma, P)
    ref = dec.decode(lch)
    dec.close()
    assert 0 < ref[1].sum() < P
    for k, v in got.items():
        for a, r in zip(v, ref):
            assert np.array_equal(a, r), (k, flag)


def test_flag0_with_compaction():
    """Early exit over a batch of 2048 (>= 1024: the grids cover the list of codewords still iterating) with flag 0: the posterior sums
    cover every codeword of the call, so outputs, flags and counts equal a decode that never polls."""
    g, meta = load_golden("osd_flag0_gf16")
    p = profile(meta)
    code = nb.Code(meta["code"])
    base = g["L_ch"]
    L = np.concatenate([base * (1.0 + 0.005 * k) for k in range(2048 // base.shape[0] + 1)])[:2048]
    kw = dict(**_method_kwargs(p), **osd_kwargs(p))
    a = nb.Decoder(code, 2, 8, **kw, poll_every=1)
    b = nb.Decoder(code, 2, 8, **kw, poll_every=0)
    ra, rb = a.decode(L), b.decode(L)
    assert 0 < ra[1].sum() < len(L)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    for i in np.flatnonzero(ra[1] == 0)[:16]:
        assert np.array_equal(a.debug_osd_sums(int(i)), b.debug_osd_sums(int(i)))
    a.close()
    b.close()
