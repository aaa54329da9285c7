"""Every field representation nbl_create accepts, on a real MI355X: the moduli of tests/field_util.py::CASES (primitive ones other than
the default, and irreducible ones that are not primitive) through every kernel family, against the CPU restatements run on the SAME
table -- the oracle loads the table file, the BS-TEMS and OSD checkers take the tables.  The kernels do not share one
multiplication (shift-and-XOR with the recovered modulus, byte lookups of the caller's table, byte offsets built from it on the
host), so each case runs on two graphs: the (2,4)-regular ring code, which selects the fused specialised / small-field kernels, and
the `all` degree profile, which selects the general kernels and the separate variable-node pass.  Three kernel variants each.
tests/test_fields.py asserts on the CPU, with the oracle alone, that every case's answer differs from the default table's: a kernel
that used a built-in constant in place of the caller's table fails here by construction.

The other consumers of the field run here on one or two shapes each: OSD (the binary image of the code from gf_mat) against the CPU
checker fed with the same matrices, and the host layer (tables loaded from SRC/ by nbldpc_sim's main loop) against a FER row of the
compiled reference run from the same directory.  The link chain over another modulus (gen, the transmitter, the error count) is
in tests/test_gpu_link_shapes.py, as two more shapes of tests/link_shapes.py."""
import json
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from conftest import GOLD, load_golden, decoder_kwargs
from bstems_util import bs_kwargs, build_checker
from degree_util import TEMS_REFUSED, spec_edges
import field_util as fu
from test_gpu_degrees import (LLR_TOL, METHODS, _force_generic, bp_frames, gpu_equals, integer_frames, literal_affordable, method_runs,
                              real_frames, reference)

pytestmark = pytest.mark.gpu

GRAPHS = ("ring", "all")
CELLS = [(q, poly, g, m) for q, poly, _ in fu.CASES for g in GRAPHS for m in METHODS if not (g == "all" and m == "tems" and ("all", q) in TEMS_REFUSED)]
FIELD_FIXTURES = ["field_gf16_m25_ems", "field_gf64_m91_tems", "field_gf256_m501_bp", "field_gf16_m25_bstems"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bstems_fields"))


def fused_expected(q, method):
    """Graph A under the default kernel choice: GF(256) and GF(64) run the fused specialised kernels, q <= 32 the fused small-field
    ones (EMS, T-EMS, log-QSPA).  GF(128) has no fused kernel, BS-TEMS has none at any q."""
    return method != "bstems" and q != 128


@pytest.mark.parametrize("q,poly,which,method", CELLS, ids=[f"gf{q}-m{poly}-{g}-{m}" for q, poly, g, m in CELLS])
def test_field_grid_vs_oracle(oracle, checker, q, poly, which, method):
    """One (q, modulus, graph, method) cell, three iterations, kernel variants 0 / 1 / 2; frames, comparisons and exclusions are
    those of tests/test_gpu_degrees.py::test_degree_grid_vs_oracle (its docstring says why each is what it is):
      * EMS (layered nc = 2, plain nc = 7), T-EMS, BS-TEMS: shaped real-valued frames bit for bit against the canonical
        restatement; integer frames with factor 1 / offset 0 against the canonical and, where affordable, the literal one; BS-TEMS
        literal on the tie-free frame only.
      * log-QSPA: decisions, flags, iteration counts equal, state within 1e-9; no partially erased and no integer frames, three
        iterations as on the grid's `all` cells (its 2-iteration graph, dc78, is not among the two graphs here).
    On the ring graph, variant 0 must have run fused (no variable-node launch) wherever a fused kernel exists."""
    gf = fu.field(q, poly)
    code, edges, _ = fu.graph(which, q, poly, method)
    rng = np.random.default_rng(100 * poly + 10 * GRAPHS.index(which) + METHODS.index(method))
    for meth, shaped, plain in method_runs(method, q):
        tag = (q, poly, which, method, tuple(shaped.values())[:1])
        if which == "ring":
            dec = nb.Decoder(code, meth, 3, fixed_iters=1, gf=gf.tables, **shaped)
            dec.decode(rng.normal(-1.5, 3.0, (2, code.N, q - 1)))
            _, (n_vn, n_syn, n_cn) = dec.last_timing()
            dec.close()
            assert (n_syn, n_cn) == (3, 3) and n_vn == (0 if fused_expected(q, method) else 3), (tag, n_vn, n_syn, n_cn)
        if method == "bp":
            L = bp_frames(rng, code.N, q)
            gpu_equals(code, meth, 3, L, {}, [reference(oracle, checker, code, edges, meth, 3, L, {}, "canonical", gf=gf)], False, tag, gf=gf)
            continue
        L = real_frames(rng, code.N, q)
        gpu_equals(code, meth, 3, L, shaped, [reference(oracle, checker, code, edges, meth, 3, L, shaped, "canonical", gf=gf)], True, tag, gf=gf)
        if meth == nb.METHOD_BS_TEMS:
            gpu_equals(code, meth, 3, L[:1], plain, [reference(oracle, checker, code, edges, meth, 3, L[:1], plain, "literal", gf=gf)], False, tag, gf=gf)
        L = integer_frames(rng, code.N, q)
        modes = ("canonical", "literal") if literal_affordable(meth, plain, int(code.chk_deg.max())) else ("canonical",)
        gpu_equals(code, meth, 3, L, plain, [reference(oracle, checker, code, edges, meth, 3, L, plain, m, gf=gf) for m in modes], True, tag, gf=gf)


@pytest.mark.parametrize("name", FIELD_FIXTURES)
def test_fixture_outputs_equal_reference(oracle, checker, name):
    """The field_* fixtures, recorded from the compiled reference run on table files of an alternative primitive modulus
    (tests/golden/make_golden_fields.py): decisions and flags equal in all three kernel variants; message state within 1e-9 of the
    reference's, and bit-identical to the canonical restatement's for EMS / T-EMS / BS-TEMS."""
    g, meta = load_golden(name)
    p = meta["profile"]
    code, edges = spec_edges(meta["spec"])
    gf = fu.field(code.q, meta["poly"])
    assert meta["poly"] != nb.datafiles.PRIMITIVE_POLY[code.q]
    meth = p["method"]
    kw = bs_kwargs(p) if meth == nb.METHOD_BS_TEMS else {} if meth == nb.METHOD_BP else \
        {k: v for k, v in decoder_kwargs(p).items() if k.startswith("ems_" if meth == nb.METHOD_EMS else "tems_")}
    L = g["L_ch"]
    for variant in (0, 1, 2):
        for k, it in enumerate(g["iters"]):
            dec = nb.Decoder(code, meth, int(it), gf=gf.tables, **kw)
            _force_generic(dec, variant)
            out, conv, iters = dec.decode(L)
            dec.close()
            assert np.array_equal(out, g["out"][k]), (name, variant, int(it))
            assert np.array_equal(conv, g["syn_ok"][k]), (name, variant, int(it))
            if meth != nb.METHOD_BP:  # (BP's failure return value is undefined in the reference)
                assert np.array_equal(conv, g["ret"][k]), (name, variant, int(it))
        for k, it in enumerate(g["state_iters"]):
            lanes = [int(b) for b in g["state_lanes"]]
            dec = nb.Decoder(code, meth, int(it), gf=gf.tables, **kw)
            _force_generic(dec, variant)
            dec.record_state(True)
            _, conv, iters = dec.decode(L)
            ref = None if meth == nb.METHOD_BP else reference(oracle, checker, code, edges, meth, int(it), L[lanes], kw, "canonical", gf=gf)
            for li, b in enumerate(lanes):
                st = dec.read_state(b)
                v_ok = not (conv[b] and iters[b] >= 2)
                for j, (a, rf) in enumerate(zip(st, (g["st_post"][k, li], g["st_v2c"][k, li], g["st_c2v"][k, li]))):
                    if j != 1 or v_ok:
                        assert np.max(np.abs(a - rf)) <= LLR_TOL * max(1.0, np.max(np.abs(rf))), (name, variant, int(it), b, j)
                        if ref is not None:
                            assert np.array_equal(a, ref[li][3][j]), (name, variant, int(it), b, j)
            dec.close()


# ---- OSD ---------------------------------------------------------------------------------------------------------------------------
OSD_PARAMS = [(n, f, a) for n, f in fu.OSD_CASES for a in (True, False)]


@pytest.fixture(scope="module")
def osd_checker(tmp_path_factory):
    from osd_util import build_checker as build_osd_checker
    return build_osd_checker(tmp_path_factory.mktemp("osd_fields"))


@pytest.mark.parametrize("name,poly,as_loaded", OSD_PARAMS, ids=[f"{n}-m{f}-{'loaded' if a else 'full'}" for n, f, a in OSD_PARAMS])
def test_osd_with_another_modulus(oracle, osd_checker, name, poly, as_loaded):
    """Two shapes of tests/osd_shapes.py over another primitive modulus, gf_mat from gf_matrices(q, poly=...) as loaded and as the
    full set: method 6 at orders 0 - 2 on 12 frames, and EMS post-processing after 1 and 2 iterations at orders 0 - 2 (flags,
    iteration counts and converged decisions from the oracle over the same field), bit for bit against the CPU checker fed with
    the same matrices.  tests/test_fields.py shows on the CPU that the default matrices give other words on these frames."""
    c = fu.osd_case(name, poly, as_loaded, osd_checker)
    code, q, gf = c["code"], c["code"].q, c["field"]
    kw = dict(gf=gf.tables, gf_mat=c["gf_mat"], **c["osd"])
    for o in fu.OSD_ORDERS:
        dec = nb.Decoder(code, nb.METHOD_OSD, 3, osd_order=o, **kw)
        out, conv, its = dec.decode(c["L"])
        dec.close()
        assert not conv.any() and not its.any(), (name, o)
        bad = [int(b) for b in range(len(out)) if not np.array_equal(out[b], c["chk"][o][0][b])]
        assert not bad, (name, poly, "method 6", o, bad, [fu.OSD_LABELS[b] for b in bad])
    for iters in (1, 2):
        r_conv, r_out, r_its = fu.osd_oracle_flags(oracle, c, iters)
        assert 0 < r_conv.sum() < len(r_conv), (name, iters, r_conv)
        for o in fu.OSD_ORDERS:
            dec = nb.Decoder(code, nb.METHOD_EMS, iters, ems_nm=min(q, 6), ems_nc=2, osd_order=o, osd_flag=1, **kw)
            out, conv, its = dec.decode(c["L"])
            dec.close()
            assert np.array_equal(conv, r_conv) and np.array_equal(its, r_its), (name, poly, iters, o)
            want = np.where((r_conv == 1)[:, None], r_out, c["chk"][o][0])
            bad = [int(b) for b in range(len(out)) if not np.array_equal(out[b], want[b])]
            assert not bad, (name, poly, iters, o, bad, [fu.OSD_LABELS[b] for b in bad])


# ---- the host layer ------------------------------------------------------------------------------------------------------------------
FER_ANCHORS = json.load(open(os.path.join(GOLD, "fer_anchors_fields.json")))
FER_KEYS = ("EbN0", "frames", "errFrame", "errSym", "errBit", "U_errFrame", "FER", "SER", "BER")


@pytest.mark.parametrize("device_tx", ["0", "1"])
@pytest.mark.parametrize("name", sorted(FER_ANCHORS))
def test_harness_reads_the_tables_of_another_modulus(tmp_path, monkeypatch, name, device_tx):
    """nbldpc_sim's main loop from a work directory whose SRC/ holds the tables of modulus 25: the host layer loads them, hands them
    to nbl_create and derives the encoder from them; every count of the row equals the compiled reference's from the same directory
    (with the host transmitter and with the device one)."""
    import link_shapes as ls
    from link_util import prepare_spec_workdir
    from nbldpc_amd import hostlib
    a = FER_ANCHORS[name]
    assert a["poly"] == ls.poly_of(name) != nb.datafiles.PRIMITIVE_POLY[a["profile"]["gfq"]]
    assert len(a["points"]) == 1 and 0 < a["points"][0]["errFrame"] < a["points"][0]["frames"]
    monkeypatch.setenv("NBL_DEVICE_TX", device_tx)
    prepare_spec_workdir(str(tmp_path), a["profile"], ls.shape(name)[1], ls.points_of(name), poly=a["poly"])
    rows = hostlib.simulate(str(tmp_path))
    assert len(rows) == 1
    for k in FER_KEYS:
        assert rows[0][k] == a["points"][0][k], (name, k, rows[0], a["points"][0])
