"""The conditions the loop cells of tests/test_gpu_idd_kinds.py must meet, on the CPU with each cell's reference alone
(tests/idd_kinds_cases.py): the kernel a cell claims is the one nbl_debug_plan names, its recorded pass counts are what the reference
computes, every cell sends frames into a second pass, every row of the table holds the full convergence mix, a float kind decides with
a margin in every iteration of every pass, and a layered reference is not the flooding one.  No GPU."""
import os
import re

import numpy as np
import pytest

import demod_general as dg
import idd_kinds_cases as kc
import idd_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernels the loop is pinned on elsewhere: ems256 and the general ems / tems through tests/test_gpu_idd.py::loop_decoder
COVERED_ELSEWHERE = {"ems256", "ems", "tems"}


@pytest.mark.parametrize("cell", sorted(kc.CELLS))
def test_the_plan_names_the_kernel_the_cell_claims(cell):
    c = kc.CELLS[cell]
    name, fusable, fused, _ = kc.plan(cell)
    assert (name, fused) == (c["kernel"], c["fused"]), (cell, name, fused)
    if c["row"] == "fused":
        assert fusable, cell                                                  # variants 1 and 2 are the same shape with the fusion switched off
        assert fused == (c["variant"] == 0)


def test_every_iterating_kernel_is_in_a_cell():
    """every kernel name of nbl_plan.h that runs iterations is claimed by a cell (and confirmed by the test above), except those the
    loop is pinned on in tests/test_gpu_idd.py"""
    text = open(os.path.join(ROOT, "nbldpc_amd", "csrc", "nbl_plan.h")).read()
    enum = text[text.index("enum NblCn {"):text.index("NBL_CN_COUNT")]
    names = {n.lower() for n in re.findall(r"\bNBL_CN_([A-Z0-9_]+)\b", re.sub(r"//[^\n]*", "", enum))} - {"none"}
    assert len(names) == 26 and {"ems_small", "bp_wide_layered", "bstems"} <= names, sorted(names)
    claimed = {kc.CELLS[cell]["kernel"] for cell in kc.CELLS}
    assert names - claimed == COVERED_ELSEWHERE - claimed, sorted(names - claimed)
    assert claimed <= names, sorted(claimed - names)


@pytest.mark.parametrize("graph", sorted(kc.GRAPHS))
def test_every_shape_has_foreign_label_bits(graph):
    """or a prior could not change an LLR and passes 2 and 3 would repeat pass 1"""
    sh = kc.shape(graph)
    assert kc.has_foreign_bits(sh) and sh["N"] <= 96, graph
    if graph != "wide256":                                                    # (an exact kind only: ties decide the same way on both sides)
        assert (sh["src"] >= 0).all(), graph                                  # every code bit is sent: no symbol has two equal channel LLRs


def test_the_cells_are_those_the_table_promises():
    assert sorted(kc.COUNTS) == sorted(kc.CELLS)
    assert all(c["B"] <= 24 and c["row"] in kc.ROWS for c in kc.CELLS.values())
    assert {cell for cell, c in kc.CELLS.items() if c["B"] < 24} == {"bp_wide", "bp_wide_layered"}
    assert {c["ref"] for c in kc.CELLS.values()} == {"exact", "float", "composition"}
    assert {cell for cell, c in kc.CELLS.items() if c["ref"] == "composition"} == {"ems_osd"}


@pytest.mark.parametrize("cell", sorted(kc.CELLS))
def test_recorded_counts_mix_and_margin(oracle, cell):
    c = kc.CELLS[cell]
    (out, conv, its, used), gap = kc.reference(cell)
    cnt = kc.counts(conv, used)
    line = f"{cell} ({c['kernel']}, sigma {c['sigma']:g}, max_iter {c['max_iter']}, B {c['B']}): pass 1 / later / never = {cnt}"
    if c["ref"] == "float":
        line += f", smallest decide gap {gap:.3e}"
    print(line)
    assert cnt == kc.COUNTS[cell], (cell, cnt)
    assert kc.hard_condition(cnt), (cell, cnt)
    assert (used[conv == 0] == kc.PASSES).all() and ((used >= 1) & (used <= kc.PASSES)).all()
    assert ((its >= 1) & (its <= c["max_iter"])).all()
    if c["ref"] == "float":
        assert gap > kc.GAP_MIN, (cell, gap)
    else:
        assert gap is None
    if cell in kc.NO_LATER:
        assert cnt[1] == 0, cell
    else:
        assert kc.full_mix(cnt) == ir.has_loop_mix(conv, used) and cnt[1] >= 1, (cell, cnt)
    if c["schedule"] != "flooding":                                           # the schedule cannot be silently ignored
        flood = kc.flooding_reference(cell)
        assert any(not np.array_equal(a, b) for a, b in zip((out, conv, its, used), flood)), cell


def test_rows_and_the_share_of_cells_without_a_later_convergence():
    later = {cell for cell, cnt in kc.COUNTS.items() if cnt[1] >= 1}
    for row in kc.ROWS:
        full = [cell for cell, c in kc.CELLS.items() if c["row"] == row and cell in later and kc.full_mix(kc.COUNTS[cell])]
        assert full, row
    without = {cell for cell, cnt in kc.COUNTS.items() if cnt[1] == 0}
    assert without == set(kc.NO_LATER), sorted(without ^ set(kc.NO_LATER))
    print(f"cells without a later-pass convergence: {sorted(without)} ({len(without)} of {len(kc.CELLS)})")
    assert 4 * len(without) <= len(kc.CELLS)
    for cell, (lo, hi) in kc.NO_LATER.items():
        assert lo < hi and lo <= kc.CELLS[cell]["sigma"] <= hi


def test_the_generalised_loop_is_the_loop_of_the_existing_cells(oracle):
    """idd_ref.loop takes a callable now: the cells of tests/test_gpu_idd.py keep the counts idd_ref.py records, and a decoder handed
    over directly gives what its callable gives"""
    recorded = {"il64_it3": (17, 3, 4), "il64_it2": (4, 1, 19), "gf256": (13, 1, 10)}
    for cell, want in recorded.items():
        _, _, _, _, (_, conv, _, used) = ir.loop_cell(cell)
        assert kc.counts(conv, used) == want, cell
    sh, rx, sigma, max_iter, ref = ir.loop_cell("il64_it2")
    code, edges, graph = ir.oracle_graph("gf64_16qam_interleaved")
    od = oracle.Decoder(oracle.Code(edges=edges), oracle.GF(code.q), oracle.EMS, max_iter, oracle.CANONICAL, fixed_iters=0, **ir.LOOP_EMS)
    again = ir.loop(ir.oracle_decode(od), graph, sh, rx, sigma, ir.MAXLOG, ir.LOOP_PASSES, ir.MAXLOG)
    for a, b in zip(again, ref):
        assert np.array_equal(a, b)
    # the ems_osd cell's flags are those of an EMS loop on the shape of il64_it3 at its own sigma
    assert kc.CELLS["ems_osd"]["graph"] == "dc2mix64" and np.array_equal(kc.shape("dc2mix64")["src"], dg.shape("gf64_16qam_interleaved")["src"])
