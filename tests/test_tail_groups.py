"""The cells of tests/tail_cases.py, checked where no device is needed: that they reach every residue of M mod G, that the kernel
choice gives each of them the packed kernel it is meant for, and that the inputs the GPU test decodes have one answer.

tests/test_gpu_tail_groups.py compares every kernel with the oracle, and a cell that fell back to the general kernel (one check per
workgroup, no packed wave at all) would pass there; the plan test is what notices."""
import numpy as np
import pytest

import nbldpc_amd as nb
from nbldpc_amd.binding import debug_plan
import tail_cases as tc
from test_gpu_parity import LLR_TOL


def test_method_numbers():
    assert (tc.METHOD_BP, tc.METHOD_EMS, tc.METHOD_TEMS) == (nb.METHOD_BP, nb.METHOD_EMS, nb.METHOD_TEMS)


def wanted_residues(G):
    """Every class 1 .. G-1 where G <= 4; 1, G/2 and G-1 where G is 8 or 16"""
    return set(range(1, G)) if G <= 4 else {1, G // 2, G - 1}


def test_residue_coverage():
    """Computed from G = 64 / q (GF(64): 4), not from the list: every cell has M mod G != 0, every (family, q) covers the residues
    above in workgroups that also hold full waves (M > G), G = 8 and 16 have one M < G (a single, mostly empty workgroup), and
    every (family, q, M) comes fused and unfused (the ring: fused) with every method of the family."""
    assert {(f, q) for f, qs in tc.FAMILIES.items() for q in qs} == {("small", 4), ("small", 8), ("small", 16), ("small", 32), ("ems64", 64), ("bp64", 64)}
    for family, qs in tc.FAMILIES.items():
        for q, (G, _) in qs.items():
            assert G == (4 if q == 64 else 64 // q), (family, q)
            mine = [c for c in tc.CELLS if (c.family, c.q) == (family, q)]
            assert mine and all(tc.group_size(c) == G and c.M % G != 0 for c in mine), (family, q)
            Ms = sorted({c.M for c in mine})
            assert {M % G for M in Ms if M > G} >= wanted_residues(G), (family, q, Ms)
            if G >= 8:
                assert any(M < G for M in Ms), (family, q, Ms)
            for M in Ms:
                got = {(c.fused, c.method) for c in mine if c.M == M}
                assert got == {(f, m) for f in tc.FAMILY_FUSED[family] for m in tc.FAMILY_METHODS[family]}, (family, q, M)
    assert tc.FAMILY_FUSED == {"small": (True, False), "ems64": (True, False), "bp64": (True,)}
    assert len({tc.cell_id(c) for c in tc.CELLS}) == len(tc.CELLS)
    # the subsets: fixed iterations on one graph per (family, fused / unfused); batch residues and the active list on one fused graph per family
    assert {(c.family, c.fused) for c in tc.FIXED_CELLS} == {(f, u) for f in tc.FAMILIES for u in tc.FAMILY_FUSED[f]}
    assert {(c.family, c.q, c.M) for c in tc.BATCH_CELLS} == {("small", 16, 5), ("ems64", 64, 5), ("bp64", 64, 7)} and all(c.fused for c in tc.BATCH_CELLS)
    assert {c.method for c in tc.BATCH_CELLS if c.family == "small"} == {"ems", "tems", "bp"}


@pytest.mark.parametrize("cell", tc.CELLS, ids=tc.cell_id)
def test_plan_names_the_packed_kernel(cell):
    """nbl_debug_plan (host arithmetic): the packed kernel under the default choice, fused exactly where the graph was built for it;
    the same kernel unfused under variant 2; the general kernel under variant 1.  The graph has the degrees the cell stands for."""
    code, edges = tc.cell_graph(cell)
    assert (code.q, code.M) == (cell.q, cell.M) and code.M % tc.group_size(cell) != 0
    assert code.M <= 31
    if cell.family == "bp64":
        assert set(code.chk_deg.tolist()) == {4} and set(code.var_deg.tolist()) == {2}
    else:
        assert set(code.chk_deg.tolist()) == set(tc.CHK_DEGS) and set(code.var_deg.tolist()) == set(tc.VAR_DEGS[cell.fused])
        # a wave of the last workgroup, and one before it where there is one, holds checks of different degrees
        G = tc.group_size(cell)
        last = code.chk_deg[(code.M // G) * G:].tolist()
        assert len(last) == code.M % G and (len(last) == 1 or len(set(last)) > 1), last
    meth, kw = tc.method_of(cell)
    plan_kw = {k: v for k, v in kw.items() if not k.endswith(("_factor", "_offset"))}
    for variant in (0, 1, 2):
        name, fusable, fused, _ = debug_plan(code, meth, force_generic=variant, **plan_kw)
        assert name == tc.planned_kernel(cell, variant), (variant, name)
        assert fusable == cell.fused and fused == (cell.fused and variant == 0), (variant, fusable, fused)
    assert tc.planned_kernel(cell, 0) == tc.planned_kernel(cell, 2) in ("ems_small", "tems_small", "bp_small", "ems64", "bp64")
    assert tc.planned_kernel(cell, 1) in ("ems", "tems", "bp")


def _agree(a, b, tag):
    """Two oracle runs of the same frames: decisions, flags and iteration counts equal, states within LLR_TOL of the largest magnitude"""
    for f, ((r0, o0, it0, st0), (r1, o1, it1, st1)) in enumerate(zip(a, b)):
        assert (r0, it0) == (r1, it1) and np.array_equal(o0, o1), (tag, f)
        for k, (x, y) in enumerate(zip(st0, st1)):
            assert np.all(np.isfinite(x)) and np.max(np.abs(x - y)) <= LLR_TOL * max(1.0, np.max(np.abs(y))), (tag, f, "post v2c c2v".split()[k])


BP_CELLS = [c for c in tc.CELLS if c.method == "bp"]


@pytest.mark.parametrize("cell", BP_CELLS, ids=tc.cell_id)
def test_log_qspa_frames_are_well_conditioned(oracle, cell):
    """A condition on the INPUTS of the log-QSPA cells, checked with the oracle alone.  These graphs are full of 4-cycles: after a few
    iterations a variable's own L_ch comes back with the opposite sign and leaves v2c entries that are zero up to rounding noise,
    whose sign then decides the damping differently in every implementation
    (tests/test_gpu_parity.py::test_field_sizes_without_a_shipped_code).  So log-QSPA runs 3 iterations, and every frame the GPU
    test decodes -- the nine state frames under early exit, the same under fixed iterations where the cell has that run, the 17- and
    24-frame mixes of the batch cells -- must get the same decisions, flags and iteration counts, and states within 1e-9, from the
    two FP64 restatements of the oracle (canonical and literal, which order their sums differently).  A frame that fails is
    replaced through tail_cases.SEED_BUMP; none is exempt and no bound moves."""
    runs = [("state", tc.state_frames(cell), tc.STATE_ITERS["bp"], 0)]
    if cell in tc.FIXED_CELLS:
        runs.append(("fixed", tc.state_frames(cell), tc.STATE_ITERS["bp"], 1))
    if cell in tc.BATCH_CELLS:
        runs += [("mix17", tc.mixed_frames(cell, 17), tc.LONG_ITERS["bp"], 0), ("mix24", tc.mixed_frames(cell, 24), tc.LONG_ITERS["bp"], 0)]
    assert tc.STATE_ITERS["bp"] == tc.LONG_ITERS["bp"] == 3
    for tag, L, iters, fixed in runs:
        _agree(tc.oracle_run(oracle, cell, L, iters, oracle.CANONICAL, fixed), tc.oracle_run(oracle, cell, L, iters, oracle.LITERAL, fixed), tag)


@pytest.mark.parametrize("cell", tc.CELLS, ids=tc.cell_id)
def test_state_frames_leave_and_stay(oracle, cell):
    """Under early exit the two strongly negative frames converge at iteration 1 and at least one other frame goes on, so a wave of
    the batch holds codewords that leave through done[b] beside codewords that stay (the oracle's flags say so)."""
    ref = tc.oracle_run(oracle, cell, tc.state_frames(cell), tc.STATE_ITERS[cell.method], state=False)
    tc.assert_leave_and_stay(ref)


@pytest.mark.parametrize("cell", tc.BATCH_CELLS, ids=tc.cell_id)
def test_mixed_frames_mix(oracle, cell):
    """The 17-frame batch and the 24-frame tile of the active list mix frames that converge at iteration 1, later, and never; tiled
    to 1032 codewords, the list of codewords still iterating after the first window is no multiple of 8 long (for every poll
    interval that leaves a second window), so the last XCD group of the second window is partly beyond the list."""
    iters = tc.LONG_ITERS[cell.method]
    for B in (17, 24):
        ref = tc.oracle_run(oracle, cell, tc.mixed_frames(cell, B), iters, state=False)
        tc.assert_mix(ref)
        if B == 24:
            tc.assert_partly_filled_list(ref, iters)
