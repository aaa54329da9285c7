"""The field cases of tests/field_util.py on the CPU: the list is the one the issue describes, and every case is worth running --
with the oracle alone, the case's table gives other check-to-variable messages than the default table on the same graph and frame,
so a kernel that used a built-in polynomial in place of the caller's table cannot pass tests/test_gpu_fields.py."""
import numpy as np
import pytest

import nbldpc_amd.datafiles as df
import field_util as fu


def test_case_list():
    assert [(q, f) for q, f, _ in fu.CASES] == [(8, 13), (16, 25), (16, 31), (32, 41), (32, 61), (64, 91), (64, 115), (64, 73),
                                               (128, 131), (128, 253), (256, 299), (256, 501), (256, 283)]
    for q, poly, kind in fu.CASES:
        assert poly != df.PRIMITIVE_POLY[q] and poly in df.irreducible_polys(q)
        assert df.is_primitive(q, poly) == (kind == "primitive")
    # a modulus that is irreducible but not primitive exists exactly where 2^p - 1 is composite
    assert {q for q, _, kind in fu.CASES if kind == "irreducible"} == {16, 64, 256}
    assert all(len(df.irreducible_polys(q)) == sum(df.is_primitive(q, f) for f in df.irreducible_polys(q)) for q in (8, 32, 128))
    assert df.irreducible_polys(4) == [7]                      # GF(4): no alternative


@pytest.mark.parametrize("q,poly,kind", fu.CASES, ids=fu.IDS)
def test_ring_graph_holds_the_coefficients_that_matter(q, poly, kind):
    code, _, _ = fu.ring_graph(q, poly)
    hs = set(code.chk_h.tolist())
    assert {1, 2, q // 2, q - 1} <= hs and hs & set(fu.inverse_differs(q, poly))
    assert (code.N, code.M) == (16, 8) and set(code.chk_deg.tolist()) == {4} and set(code.var_deg.tolist()) == {2}


@pytest.mark.parametrize("which", ["ring", "all"])
@pytest.mark.parametrize("q,poly,kind", fu.CASES, ids=fu.IDS)
def test_case_differs_from_the_default_table(oracle, q, poly, kind, which):
    """EMS, one iteration, the first real-valued frame: c2v under the default table != c2v under the case's table (oracle only)."""
    _, edges, _ = fu.graph(which, q, poly, "ems")
    L = fu.first_real_frame(edges[0], q)
    kw = dict(ems_nm=min(q, 6), ems_nc=2, ems_factor=1.15, ems_offset=0.2)
    st = []
    for gf in (oracle.GF(q), fu.field(q, poly).oracle_gf(oracle)):
        od = oracle.Decoder(oracle.Code(edges=edges), gf, oracle.EMS, 1, oracle.CANONICAL, fixed_iters=1, **kw)
        od.decode(L)
        st.append(od.state()[2].copy())
    assert not np.array_equal(st[0], st[1]), (q, poly, which)
    assert np.mean(st[0] != st[1]) > 0.05, (q, poly, which, np.mean(st[0] != st[1]))   # not one stray entry


# ---- OSD over another modulus (the cases of field_util.OSD_CASES), CPU side --------------------------------------------------------
OSD_PARAMS = [(n, f, a) for n, f in fu.OSD_CASES for a in (True, False)]
OSD_IDS = [f"{n}-m{f}-{'loaded' if a else 'full'}" for n, f, a in OSD_PARAMS]


@pytest.fixture(scope="module")
def osd_checker(tmp_path_factory):
    from osd_util import build_checker
    return build_checker(tmp_path_factory.mktemp("osd_fields"))


@pytest.mark.parametrize("name,poly,as_loaded", OSD_PARAMS, ids=OSD_IDS)
def test_osd_case_is_worth_running_and_passes_creation(oracle, osd_checker, name, poly, as_loaded):
    """What tests/test_gpu_fields.py::test_osd_with_another_modulus relies on, from the checker and the oracle alone: the matrix is
    of full row rank (asserted by osd_case), the checker fed with the DEFAULT element matrices decodes some frame to another word
    (an OSD that ignored the caller's gf_mat fails by construction), the elimination rotates and repairs pivots, winners differ from
    the base word, the batches sent to post-processing mix converged and unconverged frames -- and nbl_create_osd accepts tables
    and matrices (it fails, if at all, for want of a device)."""
    import torch
    import nbldpc_amd as nb
    import osd_shapes as sh
    from osd_util import run_checker
    assert {sh.SHAPES[n]["q"] for n, _ in fu.OSD_CASES} == {8, 16}
    c = fu.osd_case(name, poly, as_loaded, osd_checker)
    code = c["code"]
    default = df.gf_matrices(code.q, as_loaded=as_loaded)
    differs = 0
    for o in fu.OSD_ORDERS:
        out = run_checker(osd_checker, code, c["L"], o, 1, gf_mat=default, **c["osd"])
        differs += int((out != c["chk"][o][0]).any(axis=1).sum())
    assert differs > 0, (name, poly)
    cnt = c["chk"][2][1]
    assert (cnt["repairs"] > 0).any() and any(c["chk"][o][1]["differs"].any() for o in (1, 2)), (name, cnt)
    if as_loaded:    # (with the full set no column of H_bit is zero)
        assert (cnt["rotations"] > 0).any(), (name, cnt["rotations"])
    for iters in (1, 2):
        flags = fu.osd_oracle_flags(oracle, c, iters)[0]
        assert 0 < flags.sum() < len(flags), (name, poly, iters, flags)
    try:
        d = nb.Decoder(code, nb.METHOD_EMS, 2, ems_nm=4, ems_nc=2, osd_order=2, osd_flag=1, gf=c["field"].tables, gf_mat=c["gf_mat"], **c["osd"])
        assert torch.cuda.is_available()
        d.close()
    except nb.NblError as e:
        assert e.status == -3 and not torch.cuda.is_available(), (name, str(e))
