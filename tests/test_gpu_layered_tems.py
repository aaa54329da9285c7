"""The damped layered (check-serial) T-EMS schedule on a real MI355X (nbl_create_layered_ex with NBL_LAYERED_DAMPED,
nbl_cn_tems_layered.hip) against its numpy restatement (tests/layered_tems_ref.py, which takes the per-check update from the
reference-pinned oracle): out_sym, converged, iters, post, c2v and v2c of every frame, bit for bit.  Shapes are the smallest that reach
each code path: the shipped GF(16) code, ring graphs over GF(64) and GF(256) (one and four symbols per lane), the `all` degree profile
(checks 2-8, variables 1-8) over GF(4), GF(8) and GF(16) with nc = 4 (the general programme) and nc = 3 (the fast one), variables of
degree 4-8 over GF(32) and GF(256)."""
import numpy as np
import pytest

import nbldpc_amd as nb
from test_gpu_layered import assignments, case as ems_case
from test_gpu_parity import _force_generic
from test_layered import oracle_edges
from test_layered_tems import case, reference

pytestmark = pytest.mark.gpu


def equal_to(dec, got, ref, tag, B=None):
    """every output and the message state of frames 0 .. B-1 of the last decode against the restatement"""
    out, conv, its = got
    for b in range(len(ref) if B is None else B):
        r_out, r_conv, r_its, r_post, r_c2v, r_v2c = ref[b][:6]
        assert (conv[b], its[b]) == (r_conv, r_its), (tag, b, conv[b], its[b], r_conv, r_its)
        assert np.array_equal(out[b], r_out), (tag, b)
        post, v2c, c2v = dec.read_state(b)
        assert np.array_equal(post, r_post), (tag, b, "post")
        assert np.array_equal(c2v, r_c2v), (tag, b, "c2v")
        assert np.array_equal(v2c, r_v2c), (tag, b, "v2c")


def layered(name, which="greedy", **extra):
    code, kw, L, iters = case(name)
    dec = nb.Decoder(code, nb.METHOD_TEMS, iters, layers="greedy" if which == "greedy" else assignments(code)[which], damped=True, **kw, **extra)
    dec.record_state(True)
    return dec, L


def test_gf16_frames_that_converge_at_different_iterations(oracle):
    """Shipped GF(16) code, nr = 2, nc = 3, 8 frames, 6 iterations, greedy layers: frames 4, 6 and 7 converge at iterations 6, 3 and 4,
    the other five do not; iters is checked per frame, the state of a converged frame is what iteration iters - 1 left.  Launches per
    iteration: decision, syndrome, one per layer."""
    ref = reference("gf16", "greedy")
    assert [(r[1], r[2]) for r in ref] == [(0, 6), (0, 6), (0, 6), (0, 6), (1, 6), (0, 6), (1, 3), (1, 4)]
    dec, L = layered("gf16")
    equal_to(dec, dec.decode(L), ref, "gf16")
    assert np.array_equal(dec.layers, assignments(case("gf16")[0])["greedy"])
    _, (n_vn, n_syn, n_cn) = dec.last_timing()
    assert n_vn == n_syn == 6 and n_cn == 6 * (int(dec.layers.max()) + 1)
    dec.close()


@pytest.mark.parametrize("which", ["greedy", "serial", "other"])
@pytest.mark.parametrize("name", ["ring256", "ring64"])
def test_ring_codes_under_three_assignments(oracle, name, which):
    """_ring_code(256, 8, 4) and _ring_code(64, 8, 4), nr = 2, nc = 3, shaped (factor 1.15, offset 0.2): 4 frames (one with erasures),
    4 iterations, under the greedy assignment, one layer per check, and a caller's assignment that is neither.  The three references
    differ from each other and from the undamped one (tests/test_layered_tems.py)."""
    dec, L = layered(name, which)
    equal_to(dec, dec.decode(L), reference(name, which), (name, which))
    assert np.array_equal(dec.layers, assignments(case(name)[0])[which])
    dec.close()


@pytest.mark.parametrize("nr,nc", [(2, 4), (1, 3)])
@pytest.mark.parametrize("q", [4, 8, 16])
def test_small_fields_on_every_degree(oracle, q, nr, nc):
    """GF(4), GF(8), GF(16) on the `all` degree profile (checks of degree 2-8, variables of degree 1-8), nr = 2 with nc = 4 (the
    general programme: nc > 3) and nr = 1 with nc = 3 (the fast one), one frame on an integer grid (exact ties), 4 iterations."""
    name = f"all-{q}-{nr}-{nc}"
    code = case(name)[0]
    assert code.var_deg.min() == 1 and code.var_deg.max() == 8 and (code.chk_deg.min(), code.chk_deg.max()) == (2, 8)
    dec, L = layered(name)
    equal_to(dec, dec.decode(L), reference(name, "greedy"), name)
    dec.close()


@pytest.mark.parametrize("q", [32, 256])
def test_variables_of_degree_four_to_eight(oracle, q):
    """profile_code("dv48", q): variables of degree 4-8 (up to eight c2v vectors summed per input), at one and four symbols per lane."""
    name = f"dv48-{q}-2-3"
    code = case(name)[0]
    assert (code.var_deg.min(), code.var_deg.max()) == (4, 8)
    dec, L = layered(name)
    equal_to(dec, dec.decode(L), reference(name, "greedy"), name)
    dec.close()


def test_fixed_iterations(oracle):
    """fixed_iters = 1: every frame runs max_iter iterations, its outputs frozen at the first zero syndrome, its state (c2v and v2c)
    still moving; against the restatement's fixed mode."""
    ref, early = reference("gf16", "greedy", 1), reference("gf16", "greedy")
    assert any(r[1] and r[2] < 6 for r in ref)
    for r, e in zip(ref, early):
        assert (r[1], r[2]) == (e[1], e[2]) and np.array_equal(r[0], e[0])
        assert r[2] == 6 or not np.array_equal(r[5], e[5])      # (a frame that converged early went on iterating)
    dec, L = layered("gf16", fixed_iters=1)
    equal_to(dec, dec.decode(L), ref, "fixed")
    dec.close()


def test_poll_every_does_not_change_results(oracle):
    ref = reference("gf16", "greedy")
    for poll in (0, 1, 4):
        dec, L = layered("gf16", poll_every=poll)
        equal_to(dec, dec.decode(L), ref, ("poll", poll))
        dec.close()


def test_batches_of_one_and_five(oracle):
    ref = reference("gf16", "greedy")
    dec, L = layered("gf16")
    for B in (1, 5):
        equal_to(dec, dec.decode(L[:B]), ref, ("B", B), B=B)
    dec.close()


def test_device_buffers_equal_host_buffers(oracle):
    import torch
    ref = reference("gf16", "greedy")
    dec, L = layered("gf16")
    B = L.shape[0]
    dL = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    out = torch.zeros((B, dec.code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    equal_to(dec, (out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, "device")
    host = dec.decode(L)
    for a, b in zip(host, (out, conv, its)):
        assert np.array_equal(a, b.cpu().numpy())
    dec.close()


def test_damped_flag_is_inert_for_ems(oracle):
    """damped=True with METHOD_EMS is the layers-only decoder, bit for bit, on the GF(16) EMS case of tests/test_gpu_layered.py; and
    it keeps no v2c either."""
    code, kw, L, iters = ems_case("gf16")
    got = []
    for extra in (dict(), dict(damped=True), dict(damped=False)):
        dec = nb.Decoder(code, nb.METHOD_EMS, iters, layers="greedy", **kw, **extra)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        got.append((out, conv, its, [dec.read_state(b, v2c=False) for b in range(L.shape[0])]))
        with pytest.raises(nb.NblError) as e:
            dec.read_state(0, post=False)
        assert e.value.status == -2 and "v2c" in str(e.value)
        dec.close()
    assert got[0][1].any() and not got[0][1].all()
    for other in got[1:]:
        for a, b in zip(got[0][:3], other[:3]):
            assert np.array_equal(a, b)
        for sa, sb in zip(got[0][3], other[3]):
            assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[2], sb[2])


@pytest.mark.parametrize("name", ["gf16", "ring256"])
def test_flooding_decoder_is_unchanged(oracle, name):
    """A T-EMS decoder made by nbl_create on the same inputs still equals the canonical flooding oracle in every kernel variant --
    variant 1 is the general T-EMS kernels, whose check-node programmes the layered kernel shares."""
    code, kw, L, iters = case(name)
    od = oracle.Decoder(oracle.Code(edges=oracle_edges(code)), oracle.GF(code.q), oracle.TEMS, iters, oracle.CANONICAL, **kw)
    ref = []
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        ref.append((r, o.copy(), it, [x.copy() for x in od.state()]))
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, nb.METHOD_TEMS, iters, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        for b, (r, o, it, st) in enumerate(ref):
            assert (conv[b], its[b]) == (r, it) and np.array_equal(out[b], o), (name, variant, b)
            for k, (a, x) in enumerate(zip(dec.read_state(b), st)):
                if not (k == 1 and r == 1 and it >= 2):
                    assert np.array_equal(a, x), (name, variant, b, k)
        dec.close()


def test_harness_schedule_switch(tmp_path, monkeypatch):
    """NBL_SCHEDULE=layered-damped in the host layer: the harness on the shipped GF(16) code, T-EMS nr = 2 nc = 3, 6 iterations, BPSK at
    2 dB, 8 lanes.  Its counts are those of the same frames (the host link chain's, lane after lane) decoded by
    Decoder(layers="greedy", damped=True) and counted by the host chain's ErrCount.  NBL_SCHEDULE=layered still refuses a T-EMS
    profile, and an unknown schedule is named."""
    from nbldpc_amd import hostlib
    from test_layered import GF16
    code = nb.Code(GF16)
    N, K, P = code.N, code.N - code.M, 8
    kw = dict(gfq=16, method=nb.METHOD_TEMS, max_iter=6, tems_nr=2, tems_nc=3, parallel=P, crc_len=8, random_msg=1, min_sim_cycle=320,
              snr_begin=2.0, snr_step=1.0, snr_stop=2.0)
    hostlib.prepare_workdir(str(tmp_path), kw, GF16, "BPSK")
    monkeypatch.setenv("NBL_SCHEDULE", "layered-damped")
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == 1
    r = rows[0]
    frames = int(r["frames"])
    assert frames >= 320 and frames % P == 0 and 0 < r["errFrame"] < frames, r
    L, tx, msg, _ = hostlib.frontend(str(tmp_path), 2.0, frames // P, N, K, code.q, P)
    dec = nb.Decoder(code, nb.METHOD_TEMS, 6, tems_nr=2, tems_nc=3, poll_every=2, layers="greedy", damped=True)
    out, conv, its = dec.decode(L)
    dec.close()
    err_sym, err_bit, _ = hostlib.err_count(str(tmp_path), msg, out)
    print("harness", r, "own", int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum()))
    assert (r["errFrame"], r["errSym"], r["errBit"]) == (int((err_sym != 0).sum()), int(err_sym.sum()), int(err_bit.sum())), r
    flood = nb.Decoder(code, nb.METHOD_TEMS, 6, tems_nr=2, tems_nc=3, poll_every=2)
    f_out, _, f_its = flood.decode(L)
    flood.close()
    assert not np.array_equal(f_its, its)               # (the schedule in use is not flooding)
    monkeypatch.setenv("NBL_SCHEDULE", "layered")
    with pytest.raises(RuntimeError):
        hostlib.simulate(str(tmp_path))
    monkeypatch.setenv("NBL_SCHEDULE", "layered-dumped")
    with pytest.raises(RuntimeError):
        hostlib.simulate(str(tmp_path))
