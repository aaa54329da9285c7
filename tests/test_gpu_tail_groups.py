"""Check-node kernels that pack several checks into a wave, on codes whose last wave is partly empty (real MI355X).

nbl_cn_small.hip (q <= 32: 64 / q checks per wave), nbl_cn_ems64.hip and nbl_cn_bp64.hip (4 per wave) give a codeword ceil(M / G)
workgroups; with M mod G != 0 the last one holds groups without a check (`m >= g.M`), and everything behind that test is wave-level
code written with full groups in mind: ballot slices, row DPP reductions, shuffles from a group's first lane, wave fences around
per-group LDS regions, per-group divergent branches.  No shipped code and no other synthetic graph of the suite gets there at
q = 16, 32 or 64.  tests/tail_cases.py walks the residues of M mod G; here every cell runs in the three kernel variants of
nbl_debug_force_generic against the canonical oracle -- EMS and T-EMS bit for bit, log-QSPA within 1e-9 with decisions, flags and
iteration counts equal (on frames that tests/test_tail_groups.py has shown to be well conditioned) -- together with the two edges
that meet the same lines: grid slots beyond the batch (the XCD grids cover whole groups of 8 codeword slots) and beyond the active
list.  That each cell really runs the packed kernel, fused where meant, is tests/test_tail_groups.py's part (host arithmetic)."""
import numpy as np
import pytest

import nbldpc_amd as nb
import tail_cases as tc
from test_gpu_parity import LLR_TOL, _force_generic

pytestmark = pytest.mark.gpu

STATE = "post v2c c2v".split()


def compare_state(dec, cell, ref, fixed, tag):
    """Message state of every frame against the oracle's.  (v2c of a codeword that converged at iteration k >= 2 under early exit is
    not the reference's: include/nbldpc.h, nbl_read_state.)"""
    for b, (r, _, it, st) in enumerate(ref):
        for k, (a, x) in enumerate(zip(dec.read_state(b), st)):
            if k == 1 and r == 1 and it >= 2 and not fixed:
                continue
            if cell.method == "bp":
                assert np.all(np.isfinite(a)), (tag, b, STATE[k])
                assert np.max(np.abs(a - x)) <= LLR_TOL * max(1.0, np.max(np.abs(x))), (tag, b, STATE[k])
            else:
                assert np.array_equal(a, x), (tag, b, STATE[k])


def compare_outputs(got, ref, tag):
    out, conv, its = got
    assert len(ref) == out.shape[0]
    for b, (r, o, it, _) in enumerate(ref):
        assert (conv[b], its[b]) == (r, it) and np.array_equal(out[b], o), (tag, b, (conv[b], its[b]), (r, it))


def run_variants(cell, L, ref, fixed):
    code, _ = tc.cell_graph(cell)
    meth, kw = tc.method_of(cell)
    iters = tc.STATE_ITERS[cell.method]
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, meth, iters, fixed_iters=fixed, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        compare_outputs(dec.decode(L), ref, (variant,))
        compare_state(dec, cell, ref, fixed, (variant,))
        dec.close()


@pytest.mark.parametrize("cell", tc.CELLS, ids=tc.cell_id)
def test_state_parity(oracle, cell):
    """B = 9 (one full XCD group of codeword slots and a second with one codeword and seven slots beyond the batch), early exit,
    4 iterations (log-QSPA 3): real-valued frames, an integer-grid frame (ties; log-QSPA: a narrow real-valued one), an all-zero
    frame and two strongly negative frames that leave through done[b] after iteration 1 while their neighbours stay.  Decisions,
    flags, iteration counts and the message state of every frame, kernel variants 0 / 1 / 2.  One more decode per variant with
    fixed_iters = 1 (uniform windows) reads the launch counters: a fused cell makes no variable-node launch under the default choice."""
    code, _ = tc.cell_graph(cell)
    L = tc.state_frames(cell)
    assert L.shape[0] == 9
    ref = tc.oracle_run(oracle, cell, L, tc.STATE_ITERS[cell.method])
    tc.assert_leave_and_stay(ref)
    run_variants(cell, L, ref, 0)
    meth, kw = tc.method_of(cell)
    iters = tc.STATE_ITERS[cell.method]
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, meth, iters, fixed_iters=1, **kw)
        _force_generic(dec, variant)
        dec.decode(L)
        _, (n_vn, n_syn, n_cn) = dec.last_timing()
        dec.close()
        assert (n_syn, n_cn) == (iters, iters), (variant, n_vn, n_syn, n_cn)
        assert n_vn == (0 if cell.fused and variant == 0 else iters), (variant, n_vn)


@pytest.mark.parametrize("cell", tc.FIXED_CELLS, ids=tc.cell_id)
def test_fixed_iterations(oracle, cell):
    """fixed_iters = 1 on one graph per (family, fused / unfused): no group leaves early but the empty ones, and the messages of
    a converged codeword keep being updated.  Everything against the oracle's fixed-iteration run, v2c included."""
    L = tc.state_frames(cell)
    run_variants(cell, L, tc.oracle_run(oracle, cell, L, tc.STATE_ITERS[cell.method], fixed=1), 1)


@pytest.mark.parametrize("cell", tc.BATCH_CELLS, ids=tc.cell_id)
def test_batch_residues(oracle, cell):
    """Every batch size 1 .. 17 on one decoder handle: the last XCD group of the grid holds 1 .. 8 codewords beside slots beyond the
    batch, each with a partly empty last wave.  A batch decodes like the first rows of the 17-frame batch, which equals the oracle's."""
    code, _ = tc.cell_graph(cell)
    meth, kw = tc.method_of(cell)
    iters = tc.LONG_ITERS[cell.method]
    L = tc.mixed_frames(cell, 17)
    ref = tc.oracle_run(oracle, cell, L, iters, state=False)
    tc.assert_mix(ref)
    dec = nb.Decoder(code, meth, iters, **kw)
    full = dec.decode(L)
    compare_outputs(full, ref, "B = 17")
    for B in range(1, 18):
        got = dec.decode(L[:B])
        for k, (a, f) in enumerate(zip(got, full)):
            assert np.array_equal(a, f[:B]), (B, "out converged iters".split()[k])
    dec.close()


@pytest.mark.parametrize("cell", tc.BATCH_CELLS, ids=tc.cell_id)
def test_active_list(monkeypatch, oracle, cell):
    """1032 codewords (a 24-frame mix of frames that converge at iteration 1, later and never, tiled), early exit with polling: from
    the second window on the grids cover the list of codewords still iterating, whose length is no multiple of 8 (asserted on the
    oracle's iteration counts), so a partly filled XCD group has slots beyond the list -- each with a partly empty last wave.
    Poll intervals 1 and 3 with the list, 3 without (NBL_COMPACT=0), two calls per handle: all equal, and equal to the oracle's."""
    code, _ = tc.cell_graph(cell)
    meth, kw = tc.method_of(cell)
    iters = tc.LONG_ITERS[cell.method]
    tile = tc.mixed_frames(cell, 24)
    ref = tc.oracle_run(oracle, cell, tile, iters, state=False)
    tc.assert_mix(ref)
    tc.assert_partly_filled_list(ref, iters)
    L = np.concatenate([tile] * tc.TILES, axis=0)
    assert L.shape[0] == 1032
    res = {}
    for compact, poll in (("0", 3),) + tuple(("1", p) for p in tc.POLLS):
        monkeypatch.setenv("NBL_COMPACT", compact)
        dec = nb.Decoder(code, meth, iters, poll_every=poll, **kw)
        res[(compact, poll)] = dec.decode(L)
        res[(compact, poll, "again")] = dec.decode(L)          # (the list of the first call must not leak into the second)
        dec.close()
    plain = res[("0", 3)]
    assert 0.05 < plain[1].mean() < 1.0
    for key, got in res.items():
        for a, b in zip(got, plain):
            assert np.array_equal(a, b), key
    compare_outputs(tuple(a[:24] for a in plain), ref, "first tile")
