"""The C-ABI shared library: loads, exports every symbol include/nbldpc.h declares, and rejects bad arguments
with the reference's error semantics -- all without touching a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nbldpc_amd as nb
from degree_util import ring_code as _ring_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "nbldpc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nbl_[a-z_]+)\s*\(", text)))


def test_header_symbols_are_exported():
    lib = nb.load_library()
    syms = declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/nbldpc.h but not exported"
    assert sorted(nb.EXPORTS) == syms
    assert lib.nbl_abi_version() == 1


def test_no_oracle_in_product_library():
    """The product must not link or embed the CPU checker."""
    blob = open(nb.LIB_PATH, "rb").read()
    assert b"nblo_" not in blob and b"liboracle" not in blob
    for root, _, files in os.walk(os.path.join(ROOT, "nbldpc_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(root, f), errors="ignore").read()
                assert "pyoracle" not in src and "nbl_oracle" not in src, f


def _create(code, **kw):
    return nb.Decoder(code, **kw)


def test_create_rejects_bad_arguments_before_touching_the_device():
    code = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    with pytest.raises(nb.NblError) as e:
        _create(code, method=nb.METHOD_EMS, max_iter=5, ems_nm=17)  # NBLDPC.cpp:282-286
    assert e.value.status == -1 and "EMS_Nm is too large" in str(e.value)
    for method in (3, 5, 6, 7, 0):  # Min-Max, T-Min-Max: "has not been developed"; OSD / BS-TEMS out of scope
        with pytest.raises(nb.NblError) as e:
            _create(code, method=method, max_iter=5)
        assert e.value.status == -2
    # inconsistent graph: variable side and check side disagree
    bad = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    bad.var_h = bad.var_h.copy()
    bad.var_h[0] ^= 1
    with pytest.raises(nb.NblError) as e:
        _create(bad, method=nb.METHOD_EMS, max_iter=5, ems_nm=8)
    assert e.value.status == -1
    # GF(512): the reference ships arithmetic tables for it but no code; a valid request this library cannot serve (-2), not a
    # malformed one (-1)
    big = _ring_code(512, 8, 4)
    with pytest.raises(nb.NblError) as e:
        _create(big, method=nb.METHOD_EMS, max_iter=5, ems_nm=8, gf=(np.zeros((512, 512), np.uint16), np.zeros(512, np.uint16)))
    assert e.value.status == -2 and "GF(256)" in str(e.value)
    # GF table that is not a field table
    mul, inv = nb.datafiles.gf_tables(16)
    mul = [row[:] for row in mul]
    mul[3][2] ^= 1
    with pytest.raises(nb.NblError):
        _create(code, method=nb.METHOD_EMS, max_iter=5, ems_nm=8, gf=(mul, inv))


def test_no_device_means_error_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    code = nb.Code("divsalar.UNBLDPC.128.64.GF.16")
    with pytest.raises(nb.NblError) as e:
        _create(code, method=nb.METHOD_EMS, max_iter=5, ems_nm=8)
    assert e.value.status == -3 and "no CPU decode path" in str(e.value)


def test_create_refuses_shapes_the_kernels_cannot_run():
    """Limits of the kernels are refused by nbl_create with NBL_ERR_UNSUPPORTED and a message, not at the first decode."""
    code = _ring_code(256, 8, 6)                       # GF(256), check degree 6: 8 * 6 > 32
    assert code.chk_deg.max() == 6 and code.var_deg.max() == 2
    with pytest.raises(nb.NblError) as e:
        _create(code, method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=2)
    assert e.value.status == -2 and "must not exceed 32" in str(e.value)
    # (EMS at the largest supported shape -- GF(256), check degree 8, nm = q, nc = 6: 71 KB of LDS -- is accepted and run by
    #  tests/test_gpu_parity.py::test_generic_ems_beyond_64k_lds)


def _no_device():
    import torch
    return not torch.cuda.is_available()


def _accepted(code, **kw):
    """The shape checks of nbl_create precede the device: an accepted shape fails with NBL_ERR_NO_DEVICE on a box without a
    GPU and makes a decoder on one."""
    if _no_device():
        with pytest.raises(nb.NblError) as e:
            _create(code, **kw)
        assert e.value.status == -3, str(e.value)
    else:
        _create(code, **kw).close()


def _with_extra_edges(code, var, checks):
    """`code` with variable `var` joined to each of `checks` as well (coefficient 1)."""
    off = np.concatenate([[0], np.cumsum(code.var_deg)])
    var_rows = [[(int(code.var_chk[e]) + 1, int(code.var_h[e])) for e in range(off[n], off[n + 1])] for n in range(code.N)]
    var_rows[var] += [(m + 1, 1) for m in checks]
    chk_rows = [[] for _ in range(code.M)]
    for n, r in enumerate(var_rows):
        for m1, h in r:
            chk_rows[m1 - 1].append((n + 1, h))
    return nb.Code(spec=dict(N=code.N, M=code.M, q=code.q, var_rows=var_rows, chk_rows=chk_rows))


def test_create_enforces_the_degree_envelope():
    """Checks of degree 2 .. 8 and variables of degree 1 .. 8 (include/nbldpc.h): one more or one less is NBL_ERR_ARG."""
    ems = dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2)
    ring = _ring_code(16, 12, 8)                        # checks of degree 8, variables of degree 2
    assert ring.chk_deg.max() == 8
    _accepted(ring, **ems)
    nine = _with_extra_edges(ring, 0, [m for m in range(12) if m not in ring.var_chk[:2]][:1])
    assert nine.chk_deg.max() == 9 and nine.var_deg.max() == 3
    with pytest.raises(nb.NblError) as e:
        _create(nine, **ems)
    assert e.value.status == -1 and "(8)" in str(e.value)
    base = _ring_code(16, 12, 4)
    dv8 = _with_extra_edges(base, 0, [m for m in range(12) if m not in base.var_chk[:2]][:6])
    assert dv8.var_deg.max() == 8 and dv8.chk_deg.max() == 5
    _accepted(dv8, **ems)
    dv9 = _with_extra_edges(base, 0, [m for m in range(12) if m not in base.var_chk[:2]][:7])
    assert dv9.var_deg.max() == 9 and dv9.chk_deg.max() == 5
    with pytest.raises(nb.NblError) as e:
        _create(dv9, **ems)
    assert e.value.status == -1 and "(8)" in str(e.value)
    # a check of degree 1: check 0 with one variable of its own and nothing else
    lone = nb.Code(spec=dict(N=3, M=2, q=16, var_rows=[[(1, 1)], [(2, 2)], [(2, 3)]], chk_rows=[[(1, 1)], [(2, 2), (3, 3)]]))
    assert lone.chk_deg.min() == 1
    with pytest.raises(nb.NblError) as e:
        _create(lone, **ems)
    assert e.value.status == -1 and "check of degree < 2" in str(e.value)
    # a variable of degree 0
    none = nb.Code(spec=dict(N=3, M=1, q=16, var_rows=[[(1, 1)], [(1, 2)], []], chk_rows=[[(1, 1), (2, 2)]]))
    assert none.var_deg.min() == 0
    with pytest.raises(nb.NblError) as e:
        _create(none, **ems)
    assert e.value.status == -1 and "variable of degree < 1" in str(e.value)


def test_create_refuses_tems_path_codes_above_32_bits():
    """T-EMS: log2(q) * maxdc > 32 is refused -- exactly the cells tests/test_gpu_degrees.py leaves out of its grid, and every
    (q, maxdc) of the envelope beside them; 32 bits exactly (GF(16) dc 8, GF(256) dc 4) and everything below pass the shape checks."""
    from degree_util import PROFILES, QS, TEMS_REFUSED, profile_code
    tems = dict(method=nb.METHOD_TEMS, max_iter=5, tems_nr=2, tems_nc=2)
    for profile in PROFILES:
        for q in QS:
            code, _, _ = profile_code(profile, q, "tems")
            p = q.bit_length() - 1
            assert ((profile, q) in TEMS_REFUSED) == (p * int(code.chk_deg.max()) > 32), (profile, q)
            if (profile, q) in TEMS_REFUSED:
                with pytest.raises(nb.NblError) as e:
                    _create(code, **tems)
                assert e.value.status == -2 and "must not exceed 32" in str(e.value), (profile, q)
            else:
                _accepted(code, **tems)
    for q in QS:
        p = q.bit_length() - 1
        for dc in (2, 4, 6, 8):
            code = _ring_code(q, 12, dc)
            if p * dc > 32:
                with pytest.raises(nb.NblError) as e:
                    _create(code, **tems)
                assert e.value.status == -2 and "must not exceed 32" in str(e.value), (q, dc)
            else:
                _accepted(code, **tems)
    assert _ring_code(16, 12, 8).chk_deg.max() * 4 == 32 and _ring_code(256, 12, 4).chk_deg.max() * 8 == 32


def test_create_refuses_ems_shapes_above_160_kb_of_lds():
    """General EMS kernel, bytes of LDS for one check (nbl_ems_lds_bytes, nbl_kernels.hip): (maxdc q + (2 layers + 1) q + maxdc nm) 8 + maxdc nm 4 + 16
    with layers = nc + 1 below nc = maxdc - 1, else 1.  Inside the envelope the other checks of nbl_create leave (q <= 256,
    degrees <= 8, nm <= q) the largest value is 71,696 B (GF(256), check degree 8, nm = 256, nc = 6), so NO accepted shape
    reaches the 160 KB refusal: there is no 'just above' shape to create, and the one nearest to the bound must be accepted.
    The shapes one step outside the envelope are refused by the earlier checks, each with its own status."""
    def lds(q, maxdc, nm, nc):
        layers = 1 if nc >= maxdc - 1 else nc + 1
        return (maxdc * q + (2 * layers + 1) * q + maxdc * nm) * 8 + maxdc * nm * 4 + 16
    worst = max((lds(q, dc, nm, nc), q, dc, nm, nc) for q in (4, 8, 16, 32, 64, 128, 256) for dc in range(2, 9)
                for nm in (1, q // 2, q) for nc in range(0, 9))
    assert worst == (71696, 256, 8, 256, 6) and worst[0] < 160 * 1024
    _accepted(_ring_code(256, 12, 8), method=nb.METHOD_EMS, max_iter=5, ems_nm=256, ems_nc=6)
    assert lds(512, 8, 512, 6) < 160 * 1024 < lds(1024, 8, 1024, 6)   # (where the bound would bite: fields the library refuses)
    with pytest.raises(nb.NblError) as e:                             # nm above q
        _create(_ring_code(256, 12, 8), method=nb.METHOD_EMS, max_iter=5, ems_nm=257, ems_nc=6)
    assert e.value.status == -1 and "EMS_Nm is too large" in str(e.value)


def test_create_validates_the_field_tables():
    """nbl_create checks the caller's gf_mul / gf_inv in full, before anything is indexed by one of their entries and before the
    device is touched: every refusal below is NBL_ERR_ARG on a box without a GPU too, and its message names the offending entry.
    (Some kernels multiply by shift and XOR with the modulus recovered from the table, others look the table up as bytes: a table
    that is right in one column only would make them decode two different codes.)  None of these tables ever reaches a kernel."""
    import field_util as fu
    ems = dict(method=nb.METHOD_EMS, max_iter=5, ems_nm=4, ems_nc=2)

    def refused(code, mul, inv, *words):
        with pytest.raises(nb.NblError) as e:
            _create(code, gf=(mul, inv), **ems)
        assert e.value.status == -1, str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def tables(q, poly=None):
        mul, inv = nb.datafiles.gf_tables(q, poly)
        return np.array(mul, dtype=np.uint16), np.array(inv, dtype=np.uint16)

    code = _ring_code(16, 8, 4)
    mul, inv = tables(16)
    _accepted(code, gf=(mul, inv), **ems)
    bad = mul.copy(); bad[5, 9] = 16                                   # an entry >= q
    refused(code, bad, inv, "gf_mul[5][9]", "not an element")
    bad = mul.copy(); bad[3, 4], bad[3, 5] = mul[3, 5], mul[3, 4]      # two swapped entries in row 3 (column 2 untouched)
    refused(code, bad, inv, "gf_mul[3][4]", "not a polynomial-basis")
    bad = mul.copy(); bad[7, 11] = mul[7, 12]                          # not symmetric (bad[11][7] is still right)
    assert bad[11, 7] != bad[7, 11]
    refused(code, bad, inv, "gf_mul[7][11]", "not a polynomial-basis")
    bad = mul.copy(); bad[0, 6] = 1                                    # non-zero row 0
    refused(code, bad, inv, "gf_mul[0][6]", "not zero")
    bad = mul.copy(); bad[6, 0] = 1                                    # .. and column 0
    refused(code, bad, inv, "gf_mul[6][0]", "not zero")
    # the table of a reducible modulus: 21 = (x^2 + x + 1)^2.  It IS the shift-and-XOR product modulo 21; x^2 + x + 1 = 7 has no inverse
    rmul = np.zeros((16, 16), dtype=np.uint16)
    for a in range(16):
        for b in range(16):
            acc, x = 0, a
            for i in range(4):
                if (b >> i) & 1:
                    acc ^= x
                x <<= 1
                if x & 16:
                    x ^= 21
            rmul[a, b] = acc
    assert not (rmul[7] == 1).any() and 21 not in nb.datafiles.irreducible_polys(16)
    rinv = np.array([next((b for b in range(16) if rmul[a, b] == 1), 0) for a in range(16)], dtype=np.uint16)
    refused(code, rmul, rinv, "gf_inv", "gf_mul[7]", "modulus 21")     # 7: the first element without an inverse
    bad = inv.copy(); bad[9] = 16                                      # gf_inv[a] >= q
    refused(code, mul, bad, "gf_inv[9]", "not an element")
    # a wrong gf_inv at an element that labels no edge
    unused = [a for a in range(1, 16) if a not in set(code.chk_h.tolist())]
    assert unused, "every element labels an edge"
    bad = inv.copy(); bad[unused[0]] = inv[unused[0]] ^ 1 or 2
    refused(code, mul, bad, f"gf_inv[{unused[0]}]", "inconsistent")
    # GF(256): a correct entry plus 256 truncates to the right byte
    code256 = _ring_code(256, 8, 4)
    mul, inv = tables(256)
    _accepted(code256, gf=(mul, inv), **ems)
    bad = mul.copy(); bad[200, 100] += 256
    assert np.array_equal(bad.astype(np.uint8), mul.astype(np.uint8))
    refused(code256, bad, inv, "gf_mul[200][100]", "not an element")
    bad = inv.copy(); bad[255] += 256
    refused(code256, mul, bad, "gf_inv[255]", "not an element")
    # every field case is accepted: NBL_ERR_NO_DEVICE on a box without a GPU, not NBL_ERR_ARG
    for q, poly, _ in fu.CASES:
        for which in ("ring", "all"):
            c, _, _ = fu.graph(which, q, poly, "ems")
            _accepted(c, gf=fu.field(q, poly).tables, **ems)
