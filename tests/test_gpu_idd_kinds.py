"""The iterative-demapping loop (nbl_decode_batch_samples_idd / nbl_decode_batch_resident_idd; run_idd of nbl_api_demod.cpp) on every
decoder kind, on a real MI355X.  tests/test_gpu_idd.py pins the loop on flooding EMS and the general T-EMS kernel; the cells of
tests/idd_kinds_cases.py put every other kernel programme under it: the fused damped kernels, the layered kinds, FHT, the four wide
families under both schedules, BS-TEMS and OSD post-processing.  What the loop alone does to a kind: it runs the iterations on a
shrinking, gathered sub-batch, reads the c2v of the last pass for the survivors' extrinsic LLRs (a per-kind choice of buffer), and
relies on every pass starting from zero messages.

  the loop against the reference loop of the cell (exact kinds bit for bit; float kinds equal on cells whose every decision has a
      margin above 1e-6, tests/test_idd_kinds.py; BS-TEMS against the loop around its CPU checker; OSD: flags, iterations and passes
      of the EMS loop)
  the loop against the chain of public calls it is defined as: decode_samples, extrinsic soft output, decode_samples with that prior
      on the unconverged rows -- every cell; the only pin for out_sym under OSD
  batch independence, the active list at 1100 rows, state hygiene and refusals, the resident entry point, on cells of every row"""
import numpy as np
import pytest

import idd_kinds_cases as kc
import nbldpc_amd as nb
import soft_ref as sr
from test_gpu_idd import same

pytestmark = pytest.mark.gpu

ONE_PER_ROW = ["tems64", "tems_layered", "fht", "tems_wide_layered"]        # fused T-EMS, damped layered T-EMS, FHT flooding, tems_wide layered


def check_launches(dec, cell):
    """nbl_last_timing after a loop call describes the last pass's decode: no variable-node launch on a fused cell, n_layers check-node
    launches per iteration on a layered one"""
    c = kc.CELLS[cell]
    _, (vn, syn, cn) = dec.last_timing()
    assert syn >= 1, (cell, vn, syn, cn)
    if c["fused"]:
        assert vn == 0 and cn >= 1, (cell, vn, syn, cn)
    elif c["schedule"] != "flooding":
        assert cn == syn * (int(dec.layers.max()) + 1) and vn == syn, (cell, vn, syn, cn)
    else:
        assert vn == syn and cn >= 1, (cell, vn, syn, cn)


def compare(got, ref, cell, tag):
    if cell == "ems_osd":                                                     # OSD rewrites the words of unconverged frames only
        done = ref[1] == 1
        same((got[0][done],) + tuple(got[1:]), (ref[0][done],) + tuple(ref[1:]), tag)
    else:
        same(got, ref, tag)


@pytest.mark.parametrize("poll_every", [0, 2])
@pytest.mark.parametrize("cell", sorted(kc.CELLS))
def test_loop_equals_the_reference_loop(oracle, cell, poll_every):
    c = kc.CELLS[cell]
    ref, _ = kc.reference(cell)
    rx = kc.samples(cell)
    dec = kc.decoder(cell, poll_every)
    got = dec.decode_samples_idd(rx, c["sigma"], kc.PASSES, "maxlog")
    check_launches(dec, cell)
    print(f"{cell}: passes used {np.bincount(got[3], minlength=4)[1:].tolist()}, converged {int(got[1].sum())} of {len(got[1])}")
    compare(got, ref, cell, (cell, poll_every))
    two = dec.decode_samples_idd(rx, c["sigma"], 2, "maxlog")                 # fewer passes: the frames pass 3 would have taken stop at 2
    late = ref[3] == 3
    keep = ~late if cell != "ems_osd" else (~late & (ref[1] == 1))
    assert np.array_equal(two[0][keep], ref[0][keep])
    for a, b in zip(two[1:3], ref[1:3]):
        assert np.array_equal(a[~late], b[~late])
    assert (two[3][late] == 2).all() and not two[1][late].any()
    dec.close()


def chain(dec, rx, sigma, passes):
    """the loop as include/nbldpc.h defines it, from public calls: (out, converged, iters, passes_used)"""
    B = rx.shape[0]
    out, conv, its = dec.decode_samples(rx, sigma)
    out, conv, its, used = out.copy(), conv.copy(), its.copy(), np.ones(B, dtype=np.int32)
    live = np.flatnonzero(conv == 0)                                          # batch positions of the frames still unconverged
    rows = live.copy()                                                        # and their rows in the decoder's last batch
    for k in range(2, passes + 1):
        if not len(live):
            break
        _, bits = dec.soft_output("maxlog", sym=False, extrinsic=True)
        o, cv, it = dec.decode_samples(rx[live], sigma, prior=bits[rows])
        out[live], conv[live], its[live], used[live] = o, cv, it, k
        rows = np.flatnonzero(cv == 0)
        live = live[rows]
    return out, conv, its, used


@pytest.mark.parametrize("cell", sorted(kc.CELLS))
def test_loop_is_the_chain_of_public_calls(cell):
    c = kc.CELLS[cell]
    rx = kc.samples(cell)
    dec = kc.decoder(cell, 0)
    want = chain(dec, rx, c["sigma"], kc.PASSES)
    got = dec.decode_samples_idd(rx, c["sigma"], kc.PASSES, "maxlog")
    cnt = kc.counts(got[1], got[3])
    print(f"{cell}: pass 1 / later / never = {cnt}")
    same(got, want, cell)
    assert cnt[0] >= 1 and cnt[1] + cnt[2] >= 2, (cell, cnt)                  # the chain went beyond pass 1
    dec.close()


@pytest.mark.parametrize("cell", ONE_PER_ROW)
def test_every_codeword_alone_equals_its_row(oracle, cell):
    c = kc.CELLS[cell]
    ref, _ = kc.reference(cell)
    rx = kc.samples(cell)
    dec = kc.decoder(cell, 0)
    for b in range(rx.shape[0]):
        one = dec.decode_samples_idd(rx[b:b + 1], c["sigma"], kc.PASSES, "maxlog")
        same(one, [x[b:b + 1] for x in ref], (cell, b))
    dec.close()


@pytest.mark.parametrize("cell", ["bp_layered", "ems_wide_layered", "bp64"])
def test_batch_of_1100(cell):
    """the decoder's own active list (from 1024 codewords, poll_every = 2) inside every pass, with a launch per layer or a fused launch
    on the gathered sub-batch, and the gather at a ragged count"""
    c = kc.CELLS[cell]
    rx = kc.samples(cell)
    reps = 1100 // rx.shape[0] + 1
    big = np.concatenate([rx] * reps)[:1100]
    dec = kc.decoder(cell, 2)
    small = dec.decode_samples_idd(rx, c["sigma"], kc.PASSES, "maxlog")
    got = dec.decode_samples_idd(big, c["sigma"], kc.PASSES, "maxlog")
    check_launches(dec, cell)
    same(got, [np.concatenate([x] * reps)[:1100] for x in small], cell)
    dec.close()


@pytest.mark.parametrize("cell", ONE_PER_ROW + ["ems_layered"])
def test_state_after_a_loop_call(cell):
    c = kc.CELLS[cell]
    rx, sigma = kc.samples(cell), c["sigma"]
    dec = kc.decoder(cell, 2)
    before = dec.decode_samples(rx, sigma)
    soft_before = dec.soft_output("maxlog")
    state_before = dec.read_state(3, post=False, v2c=False)[2]
    dec.decode_samples_idd(rx, sigma, kc.PASSES)
    for call in (lambda: dec.soft_output("maxlog"), lambda: dec.soft_output("maxlog", extrinsic=True), lambda: dec.read_state(0, post=False, v2c=False)):
        with pytest.raises(nb.NblError) as e:
            call()
        assert e.value.status == -1 and "iterative-demapping loop" in str(e.value) and "ordinary decode call" in str(e.value)
    with pytest.raises(nb.NblError) as e:
        dec.soft_output_device("maxlog", None, 8)
    assert e.value.status == -1 and "iterative-demapping loop" in str(e.value)
    after = dec.decode_samples(rx, sigma)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    for a, b in zip(soft_before, dec.soft_output("maxlog")):
        assert sr.bits_equal(a, b)
    assert sr.bits_equal(state_before, dec.read_state(3, post=False, v2c=False)[2])
    ws = dec.workspace_bytes()
    again = dec.decode_samples_idd(rx, sigma, kc.PASSES)
    assert dec.workspace_bytes() == ws                                        # nothing grows the second time
    same(again, dec.decode_samples_idd(rx, sigma, kc.PASSES), (cell, "repeat"))
    dec.close()


@pytest.mark.parametrize("cell", ["tems_layered", "bp_wide"])
def test_resident_entry_point(cell):
    """the samples a slot holds (the device channel's, at the cell's sigma) through both entry points; the slot's samples are only read"""
    c = kc.CELLS[cell]
    sh = kc.shape(c["graph"])
    B = 48
    dec = kc.decoder(cell, 2)
    state = np.random.default_rng(9).integers(1, 30000, (B, 3)).astype(np.uint32)
    dec.channel_batch(0, np.zeros((B, sh["L"]), dtype=np.uint8), state, c["sigma"])
    rx = dec.read_slot_rx(0, 0, B)
    host = dec.decode_samples_idd(rx, c["sigma"], kc.PASSES, "maxlog")
    res = dec.decode_resident(0, c["sigma"], B, passes=kc.PASSES, soft="maxlog")
    same(res, host, (cell, "resident"))
    cnt = kc.counts(host[1], host[3])
    print(f"{cell}: pass 1 / later / never = {cnt} of {B}")
    assert cnt[0] >= 1 and cnt[1] + cnt[2] >= 2, (cell, cnt)
    assert sr.bits_equal(dec.read_slot_rx(0, 0, B), rx)
    dec.close()
