"""Ordered-statistics decoding on the GPU at the shapes no shipped code has (tests/osd_shapes.py): bit lengths that are no multiple
of 64, n < 64 and n up to 1024, GF(4) .. GF(128), k = 1 and 2, high and low rate, rows of CRC generators cut short -- every frame
bit for bit against the CPU checker tests/osd_check.cpp, which tests/test_osd_checker.py pins to the compiled reference on the same
shapes (osd_shape_*.npz; those fixtures run through the GPU here as well).

What a comparison covers is asserted, not assumed: osd_shapes.assert_coverage reads the checker's counters (rotations, pivot
repairs, the largest num_temp of a rotation, the winner's flip count, winner != base word, the winner's bit at n_dist) and the
batches sent to post-processing mix converged and unconverged frames by the oracle's flags.  The noise levels (osd_shapes.EBN0),
the seeds of the frames and of the graphs were chosen on the CPU with the oracle and the checker alone, so that these hold."""
import glob
import os

import numpy as np
import pytest

import nbldpc_amd as nb
import osd_shapes as sh
from conftest import GOLD, load_golden
from degree_util import spec_edges
from osd_util import build_checker, decide, flag0_sums, osd_kwargs, profile, run_checker
from test_gpu_degrees import method_runs

pytestmark = pytest.mark.gpu

SHAPES = sorted(sh.SHAPES)
EVERY_METHOD = ("gf8_odd", "just_over_512", "irregular")   # log-QSPA, T-EMS and BS-TEMS hand their flags and decisions to OSD here
FLAG0 = ("gf8_odd", "gf128", "just_over_512", "cap")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "osd_shape_*.npz")))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("osd_shapes"))


def ems_kw(q):
    return dict(ems_nm=min(q, 6), ems_nc=2)


def oracle_flags(oracle, c, iters):
    """EMS flags, decisions and iteration counts of every frame from the CPU oracle."""
    q = c["code"].q
    od = oracle.Decoder(oracle.Code(edges=c["edges"]), oracle.GF(q), oracle.EMS, iters, oracle.CANONICAL, **ems_kw(q))
    res = [od.decode(c["L"][b]) for b in range(c["L"].shape[0])]
    return (np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32))


def post_processing_equals(c, method, kw, iters, order, ref, tag):
    """One post-processing decode: flags and iteration counts as without OSD (`ref`), converged frames keep their decisions,
    every other frame equals the checker's OSD of its channel LLRs."""
    r_conv, r_out, r_its = ref
    dec = nb.Decoder(c["code"], method, iters, **kw, osd_order=order, osd_flag=1, **c["osd"])
    out, conv, its = dec.decode(c["L"])
    dec.close()
    assert np.array_equal(conv, r_conv) and np.array_equal(its, r_its), tag
    want = np.where((r_conv == 1)[:, None], r_out, c["chk"][order][0])
    bad = [int(b) for b in range(len(out)) if not np.array_equal(out[b], want[b])]
    assert not bad, (tag, bad, [sh.FRAME_LABELS[b] for b in bad])
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_shape_vs_checker(oracle, checker, name):
    """Method 6 at every order on all 15 frames, and EMS post-processing after 1 and 2 iterations at every order (EVERY_METHOD:
    log-QSPA, T-EMS and BS-TEMS too, parameters as test_gpu_degrees.method_runs); order 5 gives what order 3 gives."""
    c = sh.case(name, checker)
    sh.assert_coverage(name, c)
    code, q = c["code"], c["code"].q
    m6 = {}
    for o in sh.orders_of(name):
        dec = nb.Decoder(code, nb.METHOD_OSD, 3, osd_order=o, **c["osd"])
        out, conv, its = dec.decode(c["L"])
        dec.close()
        assert not conv.any() and not its.any(), (name, o)
        bad = [int(b) for b in range(len(out)) if not np.array_equal(out[b], c["chk"][o][0][b])]
        assert not bad, (name, "method 6", o, bad, [sh.FRAME_LABELS[b] for b in bad])
        m6[o] = out
    if 5 in m6:
        assert np.array_equal(m6[5], m6[3]) and np.array_equal(c["chk"][5][0], c["chk"][3][0]), name
    runs = [("ems", nb.METHOD_EMS, ems_kw(q))]
    if name in EVERY_METHOD:
        runs += [(m, *method_runs(m, q)[0][:2]) for m in ("bp", "tems", "bstems")]
    for label, method, kw in runs:
        for iters in (1, 2):
            if label == "ems":
                ref = oracle_flags(oracle, c, iters)
            else:  # flags and converged decisions of the same decoder without OSD (each method against its own oracle: test_gpu_degrees.py)
                off = nb.Decoder(code, method, iters, **kw)
                o_out, o_conv, o_its = off.decode(c["L"])
                off.close()
                ref = (o_conv, o_out, o_its)
            assert 0 < ref[0].sum() < len(ref[0]), (name, label, iters, "the batch must mix converged and unconverged frames", ref[0])
            pp = {o: post_processing_equals(c, method, kw, iters, o, ref, (name, label, iters, o)) for o in sh.orders_of(name)}
            if 5 in pp:
                assert np.array_equal(pp[5], pp[3]), (name, label, iters)


def test_winner_flip_counts_over_the_grid(checker):
    """Winners with 0, 1, 2 and 3 flips, and the kept base word, all occur among the frames test_shape_vs_checker compares."""
    seen = set()
    for name in ("gf8_odd", "gf8_trunc", "one_word", "k1", "just_over_64"):
        c = sh.case(name, checker)
        for o in c["chk"]:
            seen |= set(c["chk"][o][1]["flips"].astype(int).tolist())
    assert seen >= {-1, 0, 1, 2, 3}, seen


@pytest.mark.parametrize("name", ["gf8_trunc", "just_over_512"])
def test_batches_of_1_3_70_above_max_batch(oracle, checker, name):
    """70 codewords through a decoder with max_batch = 32 (three passes, the last one partial), then 3 and 1: every codeword
    equals the checker's (or the oracle's, where it converged)."""
    c = sh.case(name, checker)
    r_conv, r_out, r_its = oracle_flags(oracle, c, 2)
    B0 = c["L"].shape[0]
    idx = np.arange(70) % B0
    want = np.where((r_conv == 1)[:, None], r_out, c["chk"][1][0])
    dec = nb.Decoder(c["code"], nb.METHOD_EMS, 2, **ems_kw(c["code"].q), osd_order=1, osd_flag=1, max_batch=32, **c["osd"])
    for B in (70, 3, 1):
        out, conv, its = dec.decode(c["L"][idx[:B]])
        assert np.array_equal(conv, r_conv[idx[:B]]) and np.array_equal(its, r_its[idx[:B]]), (name, B)
        assert np.array_equal(out, want[idx[:B]]), (name, B)
    dec.close()


def test_device_pointer_entry_point_at_the_cap(oracle, checker):
    import torch
    c = sh.case("cap", checker)
    code = c["code"]
    r_conv, r_out, r_its = oracle_flags(oracle, c, 2)
    B = c["L"].shape[0]
    dec = nb.Decoder(code, nb.METHOD_EMS, 2, **ems_kw(code.q), osd_order=2, osd_flag=1, **c["osd"])
    dL = torch.from_numpy(np.ascontiguousarray(c["L"])).cuda()
    out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
    conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    its = torch.zeros(B, dtype=torch.int32, device="cuda")
    dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dec.close()
    assert np.array_equal(conv.cpu().numpy(), r_conv) and np.array_equal(its.cpu().numpy(), r_its)
    assert np.array_equal(out.cpu().numpy(), np.where((r_conv == 1)[:, None], r_out, c["chk"][2][0]))


@pytest.mark.parametrize("name", FLAG0)
def test_flag0_sums_and_outputs(checker, name):
    """Flag 0, factor 0.75, EMS, two iterations, order 1: S pinned bit for bit to sum_t factor^(T-t) post_t rebuilt from read_state
    of decodes with max_iter = 1 .. T (osd_acc_kernel at p = 3, 7, 3, 2), the OSD against the checker fed with that S and the
    decisions of an OSD-off decode."""
    c = sh.case(name, checker)
    code, L = c["code"], c["L"]
    kw, T, factor = ems_kw(code.q), 2, 0.75
    B = L.shape[0]
    posts = {}
    for t in range(1, T + 1):
        d = nb.Decoder(code, nb.METHOD_EMS, t, **kw)
        d.record_state(True)
        d.decode(L)
        posts[t] = [d.read_state(b)[0] for b in range(B)]
        d.close()
    off = nb.Decoder(code, nb.METHOD_EMS, T, **kw)
    o_out, o_conv, _ = off.decode(L)
    off.close()
    dec = nb.Decoder(code, nb.METHOD_EMS, T, **kw, osd_order=1, osd_flag=0, osd_factor=factor, **c["osd"])
    out, conv, _ = dec.decode(L)
    bad = np.flatnonzero(conv == 0)
    assert 0 < len(bad) < B and np.array_equal(conv, o_conv)
    S = np.zeros((len(bad), c["info"]["n"]))
    for j, b in enumerate(bad):
        S[j] = dec.debug_osd_sums(int(b)).reshape(-1)
        assert np.array_equal(S[j], flag0_sums([posts[t][b] for t in range(1, T + 1)], factor)), (name, b)
        assert np.array_equal(o_out[b], decide(posts[T][b])), (name, b)
    dec.close()
    c_out = run_checker(checker, code, L[bad], 1, 0, S=S, base=o_out[bad], **c["osd"])
    assert np.array_equal(out[bad], c_out), name
    assert np.array_equal(out[conv == 1], o_out[conv == 1]), name


@pytest.mark.parametrize("name", ["gf8_odd", "cap"])
def test_non_finite_inputs_terminate_with_osd(checker, name):
    """NaN, +-inf and 1e300 frames with OSD on (method 6 and EMS post-processing, order 1): the call returns, outputs lie in
    0 .. q - 1, and the finite frames of the batch decode as without the others (codewords never interact)."""
    c = sh.case(name, checker)
    code = c["code"]
    L = c["L"][:8].copy()
    bad = L.copy()
    bad[1, :, ::3] = np.nan
    bad[3, ::2, :] = np.inf
    bad[5, :, 1::2] = -np.inf
    bad[6] *= 1e300
    for method, kw in ((nb.METHOD_OSD, {}), (nb.METHOD_EMS, ems_kw(code.q))):
        dec = nb.Decoder(code, method, 2, **kw, osd_order=1, osd_flag=1, **c["osd"])
        ref = dec.decode(L)
        out, conv, its = dec.decode(bad)
        dec.close()
        for b in (0, 2, 4, 7):
            assert np.array_equal(out[b], ref[0][b]) and conv[b] == ref[1][b] and its[b] == ref[2][b], (name, method, b)
        assert out.min() >= 0 and out.max() < code.q, (name, method)


@pytest.mark.parametrize("name", FIXTURES)
def test_shape_fixture_outputs_equal_reference(name):
    """The osd_shape_* fixtures of the compiled reference: method 6 and EMS post-processing (flag 1, or flag 0 with factor 0.75) at
    every recorded order, outputs and flags."""
    g, meta = load_golden(name)
    p = profile(meta)
    code, _ = spec_edges(meta["spec"])
    okw = osd_kwargs(p)
    kw = dict(ems_nm=p["ems_nm"], ems_nc=p["ems_nc"])
    for o in g["orders"]:
        o = int(o)
        okw["osd_order"] = o
        L = g["L_ch"][:g[f"out_o{o}"].shape[1]]
        if p["osd_flag"] == 1:
            dec = nb.Decoder(code, nb.METHOD_OSD, 1, **okw)
            out, conv, its = dec.decode(L)
            dec.close()
            assert np.array_equal(out, g[f"out_m6_o{o}"]) and not conv.any(), (name, o)
        for k, it in enumerate(g["iters"]):
            dec = nb.Decoder(code, nb.METHOD_EMS, int(it), **kw, **okw)
            out, conv, its = dec.decode(L)
            dec.close()
            assert np.array_equal(out, g[f"out_o{o}"][k]), (name, o, int(it))
            assert np.array_equal(conv, g[f"ret_o{o}"][k]), (name, o, int(it))
