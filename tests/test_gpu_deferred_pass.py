"""The deferred check-node pass of the last iteration on a real MI355X ("The last check-node pass is deferred").

Undamped fused EMS runs iteration max_iter as its variable-node half alone (vn_decide on the c2v of iteration max_iter - 1) plus the
syndrome, and leaves the fused launch to the first reader of the message state (nbl_read_state's c2v, nbl_soft_output*).  Here:
outputs with nbl_debug_defer_last on and off, the launch counters, the state a reader gets (bit for bit the canonical oracle's, and
the same bytes on a second read), the conditions that switch deferral off, a pending pass that is dropped by the next decode, early
exit with frames that converge early, exactly at max_iter and never, fixed iterations whose first zero syndrome falls at max_iter,
and a decode on a caller's stream.

Two shapes, the smallest that reach the two fused undamped kernels: divsalar.UNBLDPC.128.64.GF.256 (N = 16, M = 8; EMS nm = 16,
nc = 3; nbl_cn_ems256.hip) on 24 frames of the host link chain, and the GF(16) cell of tests/tail_cases.py with variable degrees
(2, 3) and M = 5 (N = 8; nbl_cn_small.hip) on 24 BPSK frames across its waterfall.  Eb/N0 and seeds were picked with the oracle on the
CPU so that the early-exit mix exists at max_iter = 6; the tests assert the mix.

Launch counters: a profiled call counts the check-node launches its times cover (include/nbldpc.h, nbl_last_timing), which is what
the counts below are read from; an unprofiled call reports the passes of its schedule."""
import numpy as np
import pytest

import nbldpc_amd as nb
import nbldpc_amd.datafiles as df
import tail_cases as tc

pytestmark = pytest.mark.gpu

U256 = "divsalar.UNBLDPC.128.64.GF.256"
KW256 = dict(ems_nm=16, ems_nc=3, ems_factor=1.0, ems_offset=0.0)
CELL16 = tc.Cell("small", 16, 5, True, "ems")
CASES = ["gf256", "gf16"]
B = 24
EXIT_ITERS = 6


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """case -> (nb.Code, oracle edge tuple, method, parameters, frames [24][N][q-1], read-only)"""
    from nbldpc_amd import hostlib
    d = str(tmp_path_factory.mktemp("link"))
    c = df.codes()[U256]
    hostlib.prepare_workdir(d, dict(gfq=256, code=U256, method=2, max_iter=EXIT_ITERS, parallel=B, ems_nm=16, ems_nc=3, constellation="BPSK",
                                    random_msg=1, seed=1), U256, "BPSK")
    L256, _, _, _ = hostlib.frontend(d, 1.5, 1, c["N"], c["N"] - c["M"], c["q"], B)
    code16, edges16 = tc.cell_graph(CELL16)
    meth16, kw16 = tc.method_of(CELL16)
    rng = np.random.default_rng([3, 16])
    L16 = np.concatenate([tc.bpsk_zero_llr(rng, code16.N, 16, B // len(tc.MIX_EBN0), e) for e in tc.MIX_EBN0])
    for L in (L256, L16):
        assert L.shape[0] == B
        L.setflags(write=False)
    return {"gf256": (nb.Code(U256), df.code_edges(U256), nb.METHOD_EMS, KW256, L256),
            "gf16": (code16, edges16, meth16, kw16, L16)}


_REF = {}


def reference(oracle, shapes, case, max_iter, fixed):
    """[(flag, decisions, iterations, c2v)] of the case's frames from the canonical oracle: computed once per (case, max_iter, fixed)"""
    key = (case, max_iter, fixed)
    if key not in _REF:
        _, edges, meth, kw, L = shapes[case]
        od = oracle.Decoder(oracle.Code(edges=tuple(edges)), oracle.GF(edges[2]), meth, max_iter, oracle.CANONICAL, fixed_iters=fixed, **kw)
        ref = []
        for b in range(L.shape[0]):
            r, o, it = od.decode(L[b])
            ref.append((r, o.copy(), it, od.state()[2].copy()))
        _REF[key] = ref
    return _REF[key]


def decoder(shapes, case, max_iter, defer=True, fixed=1, poll=0, profiled=True):
    code, _, meth, kw, _ = shapes[case]
    dec = nb.Decoder(code, meth, max_iter, fixed_iters=fixed, poll_every=poll, **kw)
    dec.defer_last(defer)
    dec.profiling(profiled)
    return dec


def c2v_of(dec, b):
    return dec.read_state(b, post=False, v2c=False)[2]


def assert_outputs(got, ref, tag, rows=None):
    out, conv, its = got
    rows = range(len(ref)) if rows is None else rows
    for k, b in enumerate(rows):
        r, o, it, _ = ref[b]
        assert (conv[k], its[k]) == (r, it) and np.array_equal(out[k], o), (tag, b, conv[k], its[k], r, it)


def assert_c2v(dec, ref, tag, rows=None):
    rows = range(len(ref)) if rows is None else rows
    for k, b in enumerate(rows):
        assert np.array_equal(c2v_of(dec, k), ref[b][3]), (tag, b)


@pytest.mark.parametrize("max_iter", [1, 2, 3, 8])
@pytest.mark.parametrize("case", CASES)
def test_outputs_and_launch_counts_with_and_without_deferral(oracle, shapes, case, max_iter):
    L = shapes[case][4]
    ref = reference(oracle, shapes, case, max_iter, 1)
    got = {}
    for defer in (True, False):
        dec = decoder(shapes, case, max_iter, defer)
        got[defer] = dec.decode(L)
        ms, (n_vn, n_syn, n_cn) = dec.last_timing()
        dec.close()
        assert_outputs(got[defer], ref, (case, max_iter, defer))
        assert n_cn == (max_iter - 1 if defer and max_iter >= 2 else max_iter), (case, max_iter, defer, n_cn)
        assert (n_vn, n_syn) == (0, max_iter) and ms[0] == 0.0, (case, max_iter, defer, n_vn, n_syn, ms)
    for a, b in zip(got[True], got[False]):
        assert np.array_equal(a, b), (case, max_iter)
    # an unprofiled call reports its schedule: one check-node pass per iteration, run or owed
    dec = decoder(shapes, case, max_iter, True, profiled=False)
    dec.decode(L)
    assert dec.last_timing()[1] == [0, max_iter, max_iter]
    dec.close()


@pytest.mark.parametrize("max_iter", [2, 5])
@pytest.mark.parametrize("case", CASES)
def test_state_read_back_completes_the_pass_once(oracle, shapes, case, max_iter):
    L = shapes[case][4]
    ref = reference(oracle, shapes, case, max_iter, 1)
    dec = decoder(shapes, case, max_iter)
    dec.decode(L)
    assert dec.last_timing()[1][2] == max_iter - 1
    first = [c2v_of(dec, b) for b in range(B)]
    assert dec.last_timing()[1][2] == max_iter
    for b in range(B):
        assert np.array_equal(first[b], ref[b][3]), (case, max_iter, b)
        assert c2v_of(dec, b).tobytes() == first[b].tobytes(), (case, max_iter, b, "second read")
    assert dec.last_timing()[1][2] == max_iter, "further reads launch nothing"
    # soft output as the first reader, against the decoder that never defers
    off = decoder(shapes, case, max_iter, False)
    off.decode(L)
    for metric, extrinsic in (("maxlog", False), ("logsum", True)):
        dec.decode(L)
        assert dec.last_timing()[1][2] == max_iter - 1
        sym, bits = dec.soft_output(metric, extrinsic=extrinsic)
        assert dec.last_timing()[1][2] == max_iter
        o_sym, o_bits = off.soft_output(metric, extrinsic=extrinsic)
        assert sym.tobytes() == o_sym.tobytes() and bits.tobytes() == o_bits.tobytes(), (case, max_iter, metric)
        sym2, _ = dec.soft_output(metric, extrinsic=extrinsic)
        assert sym2.tobytes() == sym.tobytes() and dec.last_timing()[1][2] == max_iter
    assert off.last_timing()[1][2] == max_iter
    off.close()
    dec.close()


@pytest.mark.parametrize("case", CASES)
def test_state_recording_switches_deferral_off(oracle, shapes, case):
    code, edges, meth, kw, L = shapes[case]
    max_iter = 3
    dec = decoder(shapes, case, max_iter)
    dec.record_state(True)
    got = dec.decode(L)
    assert dec.last_timing()[1] == [0, max_iter, max_iter], "nothing deferred"
    assert_outputs(got, reference(oracle, shapes, case, max_iter, 1), (case, "record"))
    od = oracle.Decoder(oracle.Code(edges=tuple(edges)), oracle.GF(edges[2]), meth, max_iter, oracle.CANONICAL, fixed_iters=1, **kw)
    for b in (0, B // 2, B - 1):
        od.decode(L[b])
        for x, y in zip(dec.read_state(b), od.state()):
            assert np.array_equal(x, y), (case, b)
    assert dec.last_timing()[1][2] == max_iter
    dec.close()


@pytest.mark.parametrize("case", CASES)
def test_pending_pass_is_dropped_by_the_next_decode(oracle, shapes, case):
    """decode, then decode another batch without any read: same size, smaller, larger (the workspace grows)"""
    L = shapes[case][4]
    max_iter = 4
    ref = reference(oracle, shapes, case, max_iter, 1)
    dec = decoder(shapes, case, max_iter)
    for rows in (range(12, 24), range(3, 8), range(0, 24)):
        rows = list(rows)
        dec.decode(L[:12])  # leaves a pending pass that nobody reads
        got = dec.decode(L[rows])
        assert dec.last_timing()[1][2] == max_iter - 1
        assert_outputs(got, ref, (case, rows[0], len(rows)), rows)
        assert_c2v(dec, ref, (case, rows[0], len(rows)), rows)
        assert dec.last_timing()[1][2] == max_iter
    dec.decode(L[:12])
    dec.close()  # (with a pass pending)


def _mix(ref):
    its = [it if r else 0 for r, _, it, _ in ref]
    return [b for b, i in enumerate(its) if 0 < i < EXIT_ITERS], [b for b, i in enumerate(its) if i == EXIT_ITERS], [b for b, i in enumerate(its) if i == 0]


@pytest.mark.parametrize("case", CASES)
def test_early_exit_mix(oracle, shapes, case):
    L = shapes[case][4]
    ref = reference(oracle, shapes, case, EXIT_ITERS, 0)
    early, exact, never = _mix(ref)
    assert early and exact and never, (case, early, exact, never)
    state = {}
    for defer in (True, False):
        dec = decoder(shapes, case, EXIT_ITERS, defer, fixed=0, poll=2)
        got = dec.decode(L)
        assert_outputs(got, ref, (case, defer))
        state[defer] = [c2v_of(dec, b) for b in range(B)]
        for b in range(B):
            assert np.array_equal(state[defer][b], ref[b][3]), (case, defer, b)
        dec.close()
    for b in range(B):
        assert state[True][b].tobytes() == state[False][b].tobytes(), (case, b)


@pytest.mark.parametrize("case", CASES)
def test_fixed_iterations_first_zero_syndrome_at_max_iter(oracle, shapes, case):
    """the late launch sees done[] one syndrome later than the skipped one would have: a frame whose first zero syndrome falls at
    max_iter takes the short-list path there (GF(256)), which must give the same c2v"""
    L = shapes[case][4]
    early, exact, _ = _mix(reference(oracle, shapes, case, EXIT_ITERS, 0))
    assert early and exact
    ref = reference(oracle, shapes, case, EXIT_ITERS, 1)
    assert all(ref[b][0] == 1 and ref[b][2] == EXIT_ITERS for b in exact) and all(ref[b][0] == 1 and ref[b][2] < EXIT_ITERS for b in early)
    dec = decoder(shapes, case, EXIT_ITERS)
    got = dec.decode(L)
    assert dec.last_timing()[1][2] == EXIT_ITERS - 1
    assert_outputs(got, ref, (case, "fixed"))
    assert_c2v(dec, ref, (case, "fixed"))
    dec.close()


def test_decode_on_a_callers_stream(oracle, shapes):
    import torch
    code, _, _, _, L = shapes["gf256"]
    max_iter = 3
    ref = reference(oracle, shapes, "gf256", max_iter, 1)
    dec = decoder(shapes, "gf256", max_iter)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dL = torch.from_numpy(np.array(L)).cuda()
        out = torch.zeros((B, code.N), dtype=torch.int32, device="cuda")
        conv = torch.zeros(B, dtype=torch.uint8, device="cuda")
        its = torch.zeros(B, dtype=torch.int32, device="cuda")
        stream.synchronize()
        dec.decode_device(dL.data_ptr(), B, out.data_ptr(), conv.data_ptr(), its.data_ptr(), stream.cuda_stream)
    assert dec.last_timing()[1][2] == max_iter - 1
    assert_c2v(dec, ref, "stream")  # (the pending pass waits for the decode's end on the caller's stream)
    assert dec.last_timing()[1][2] == max_iter
    stream.synchronize()
    assert_outputs((out.cpu().numpy(), conv.cpu().numpy(), its.cpu().numpy()), ref, "stream")
    dec.close()
