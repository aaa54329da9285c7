"""nbl_create_osd (include/nbldpc.h): every refusal happens at creation, before any device call, so these run without a GPU."""
import numpy as np
import pytest

import nbldpc_amd as nb
from bstems_util import ring_code

U128 = "divsalar.UNBLDPC.128.64.GF.16"


def _create(code, method=nb.METHOD_EMS, **kw):
    return nb.Decoder(code, method, 5, ems_nm=8, ems_nc=2, **kw)


def _refused(code, status, text=None, **kw):
    with pytest.raises(nb.NblError) as e:
        _create(code, **kw)
    assert e.value.status == status, str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def test_library_exports_nbl_create_osd():
    assert "nbl_create_osd" in nb.EXPORTS and hasattr(nb.load_library(), "nbl_create_osd")
    assert nb.METHOD_OSD == 6


def test_create_and_create_ex_still_refuse_method_6():
    code = nb.Code(U128)
    _refused(code, -2, method=nb.METHOD_OSD)
    _refused(code, -2, "nbl_create_osd", method=nb.METHOD_OSD, bs_nm=4)


@pytest.mark.parametrize("method", [nb.METHOD_EMS, nb.METHOD_OSD])
def test_bad_osd_parameters_are_refused(method):
    code = nb.Code(U128)
    _refused(code, -1, "order < -1", method=method, osd_order=-2)
    _refused(code, -1, "flag", method=method, osd_order=1, osd_flag=2)
    _refused(code, -1, "flag", method=method, osd_order=1, osd_flag=-1)
    _refused(code, -1, "crc_rows", method=method, osd_order=1, crc_len=8, crc_rows=9)
    _refused(code, -1, "crc_rows", method=method, osd_order=1, crc_len=8, crc_rows=-1)
    _refused(code, -1, "8, 16 or 24", method=method, osd_order=1, crc_len=12, crc_rows=4)


def test_null_gf_mat_is_refused():
    import ctypes as C
    from nbldpc_amd import binding as B
    lib = nb.load_library()
    code = nb.Code(U128)
    mul, inv = nb.datafiles.gf_tables(16)
    mul = np.ascontiguousarray(np.array(mul, dtype=np.uint16))
    inv = np.ascontiguousarray(np.array(inv, dtype=np.uint16))
    prm = B.Params(nb.METHOD_EMS, 5, 8, 2, 1.0, 0.0, 2, 3, 1.0, 0.0, 0, 0, 0)
    osd = B.OsdParams(1, 1, 0.0, 8, 0, None)
    h = C.c_void_p()
    desc = code.desc()
    rc = lib.nbl_create_osd(C.byref(desc), mul.ctypes.data, inv.ctypes.data, C.byref(prm), None, C.byref(osd), 0, C.byref(h))
    assert rc == -1 and b"gf_mat" in lib.nbl_last_error(None)


def test_gf_mat_whose_element_1_is_not_the_identity_is_refused():
    """Multiplying by 1 changes nothing: whatever basis gf_mat is written in, the matrix of element 1 is the identity.  One cleared
    diagonal entry, one stray entry, and the set shifted by one element (a table indexed by the exponent instead of the element)."""
    code = nb.Code(U128)
    good = nb.datafiles.gf_matrices(16)
    for method in (nb.METHOD_EMS, nb.METHOD_OSD):
        m = good.copy()
        m[1, 2, 2] = 0
        _refused(code, -1, "element 1 is not the identity (entry [2][2])", method=method, osd_order=1, gf_mat=m)
        m = good.copy()
        m[1, 0, 3] = 1
        _refused(code, -1, "element 1 is not the identity (entry [0][3])", method=method, osd_order=1, gf_mat=m)
        _refused(code, -1, "element 1 is not the identity", method=method, osd_order=1, gf_mat=np.roll(good, 1, axis=0))
    # and the matrices of another primitive modulus pass this check with their own tables
    import torch
    alt = nb.datafiles.gf_matrices(16, poly=25)
    assert np.array_equal(alt[1], np.eye(4, dtype=np.uint8)) and not np.array_equal(alt, good)
    gf = tuple(np.array(t, dtype=np.int64) for t in nb.datafiles.gf_tables(16, 25))
    try:
        _create(code, osd_order=1, gf=gf, gf_mat=alt).close()
        assert torch.cuda.is_available()
    except nb.NblError as e:
        assert e.status in (-3, -2) and "identity" not in str(e) and (e.status == -2 or not torch.cuda.is_available()), str(e)
        assert e.status == -3 or "full row rank" in str(e), str(e)


def test_rank_deficient_matrix_is_refused():
    """Two identical check rows: [CRC rows; H_bit] loses full row rank; the reference's elimination would never end."""
    q = 16
    var_rows = [[] for _ in range(6)]
    chk_rows = [[], [], []]
    for m, vs in enumerate(([0, 1, 2, 3], [0, 1, 2, 3], [2, 3, 4, 5])):
        for v in vs:
            h = 1 + v
            var_rows[v].append((m + 1, h))
            chk_rows[m].append((v + 1, h))
    code = nb.Code(spec=dict(N=6, M=3, q=q, var_rows=var_rows, chk_rows=chk_rows))
    full = nb.datafiles.gf_matrices(q, as_loaded=False)
    _refused(code, -2, "full row rank", osd_order=0, gf_mat=full)
    _refused(code, -2, "full row rank", method=nb.METHOD_OSD, osd_order=0, gf_mat=full)


def test_matrix_above_the_lds_cap_is_refused():
    code = ring_code(256, 65, 4)  # N = 130 symbols of 8 bits: 1040 > NBL_OSD_MAX_BITS
    assert code.N * 8 > 1024
    _refused(code, -2, "NBL_OSD_MAX_BITS", osd_order=0)


@pytest.mark.parametrize("name", ["BDS.576.288.GF.64", "divsalar.UNBLDPC.512.256.GF.256", "divsalar.UNBLDPC.512.256.GF.16",
                                  "divsalar.CNBLDPC.512.256.GF.256", "divsalar.UNBLDPC.128.64.GF.16"])
def test_shipped_codes_pass_every_creation_check(name):
    """A shipped code with OSD on fails, if at all, only for want of a device (-3), never on a check."""
    import torch
    code = nb.Code(name)
    for crc_len, crc_rows in ((8, 0), (8, 8), (24, 24)):
        try:
            d = _create(code, osd_order=2, crc_len=crc_len, crc_rows=crc_rows)
            assert torch.cuda.is_available()
            d.close()
        except nb.NblError as e:
            assert e.status == -3 and not torch.cuda.is_available(), (name, crc_rows, str(e))
