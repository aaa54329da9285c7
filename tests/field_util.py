"""The field representations the C ABI accepts besides the default one: for every q the case list names moduli other than
nbldpc_amd/datafiles.py::PRIMITIVE_POLY[q], and Field carries the tables of one of them to every consumer -- nbl_create (tables),
the BS-TEMS and OSD checkers (tables, gf_mat) and the oracle (a table file written by write_gf_tables and LOADED by oracle.GF, the
way the reference gets its field, not rebuilt from the default polynomial).

CASES is computed, not written down: for q = 8 .. 256 the smallest primitive polynomial other than the default, the largest
primitive polynomial, and the smallest irreducible polynomial that is not primitive where one exists.  One exists for q = 16 (31),
q = 64 (73) and q = 256 (283, the AES modulus); at q = 8, 32 and 128 every irreducible polynomial is primitive, because 2^p - 1 (7,
31, 127) is prime and every non-zero element but 1 generates the group.  GF(4) has ONE irreducible polynomial of degree 2 (7), so
it has no alternative and no case.  At q = 8 and q = 16 the smallest other and the largest primitive polynomial coincide (13, 25).

A modulus that is not primitive is in scope on purpose: the decoders need a field, not a generator, and no kernel may take x for
one.  Such a modulus rests on the restatements alone -- the compiled reference's loader wants a Mat.Repr file that lists every
non-zero element as a power of x, which only a primitive modulus provides, so the fixtures of tests/golden/make_golden_fields.py
use primitive moduli."""
import functools
import os
import tempfile

import numpy as np

import nbldpc_amd.datafiles as df

QS = (8, 16, 32, 64, 128, 256)


@functools.lru_cache(maxsize=None)
def cases():
    """[(q, poly, kind)], kind in 'primitive' | 'irreducible' (irreducible and NOT primitive)"""
    out = []
    for q in QS:
        irr = df.irreducible_polys(q)
        prim = [f for f in irr if df.is_primitive(q, f)]
        assert df.PRIMITIVE_POLY[q] in prim
        others = [f for f in prim if f != df.PRIMITIVE_POLY[q]]
        picks = [(others[0], "primitive")]
        if prim[-1] not in (others[0], df.PRIMITIVE_POLY[q]):
            picks.append((prim[-1], "primitive"))
        rest = [f for f in irr if f not in prim]
        if rest:
            picks.append((rest[0], "irreducible"))
        out += [(q, f, kind) for f, kind in picks]
    return out


CASES = cases()
IDS = [f"gf{q}-m{poly}" for q, poly, _ in CASES]

_TMP = None


class Field:
    """GF(q) in the polynomial basis of `poly`: .tables = (mul, inv) for nbl_create and the checkers, .gf_mat(as_loaded) for OSD
    (primitive moduli), .oracle_gf(oracle) = the oracle's field LOADED from the table file write_gf_tables wrote."""

    def __init__(self, q, poly):
        self.q, self.poly = q, poly
        mul, inv = df.gf_tables(q, poly)
        self.tables = (np.array(mul, dtype=np.int64), np.array(inv, dtype=np.int64))
        self._ogf = None

    def src_dir(self):
        global _TMP
        if _TMP is None:
            _TMP = tempfile.TemporaryDirectory(prefix="fields_")
        d = os.path.join(_TMP.name, f"gf{self.q}_m{self.poly}")
        if not os.path.isdir(d):
            df.write_gf_tables(self.q, d, self.poly)
        return d

    def oracle_gf(self, oracle):
        if self._ogf is None:
            g = oracle.GF(self.q, arith_path=os.path.join(self.src_dir(), f"Arith.Table.GF.{self.q}.txt"))
            assert np.array_equal(g.mul, self.tables[0]) and np.array_equal(g.inv[1:], self.tables[1][1:])
            assert g.s.poly == self.poly       # the loader names the table's own modulus
            self._ogf = g
        return self._ogf

    def gf_mat(self, as_loaded=True):
        return df.gf_matrices(self.q, as_loaded=as_loaded, poly=self.poly)


@functools.lru_cache(maxsize=None)
def field(q, poly):
    return Field(q, poly)


def inverse_differs(q, poly):
    """elements whose inverse under `poly` is not their inverse under the default polynomial"""
    a, b = df.gf_tables(q, poly)[1], df.gf_tables(q)[1]
    return [e for e in range(1, q) if a[e] != b[e]]


def ring_graph(q, poly, seed=0):
    """Graph A: the (2,4)-regular ring code tests/bstems_util.py::ring_code(q, 8, 4) -- 8 checks of degree 4, 16 variables of
    degree 2 -- with its coefficients replaced, edge by edge in variable-major order, by draws from a seeded stream, the first five
    set to 1, 2, q / 2, q - 1 and the smallest element whose inverse differs between the default table and the table of `poly`.
    Returns (nb.Code, oracle edges, spec)."""
    from bstems_util import ring_code
    from degree_util import spec_edges
    ring = ring_code(q, 8, 4)
    N, M = ring.N, ring.M
    rng = np.random.default_rng(90000 + 1000 * q + poly + 7919 * seed)
    diff = inverse_differs(q, poly)
    assert diff, (q, poly)
    forced = [1, 2, q // 2, q - 1, diff[0]]
    chk_rows = [[] for _ in range(M)]
    var_rows = [[] for _ in range(N)]
    e = 0
    for n in range(N):
        for _ in range(int(ring.var_deg[n])):
            m = int(ring.var_chk[e])
            h = forced[e] if e < len(forced) else int(rng.integers(1, q))
            e += 1
            var_rows[n].append((m + 1, h))
            chk_rows[m].append((n + 1, h))
    spec = dict(N=N, M=M, q=q, var_rows=var_rows, chk_rows=chk_rows)
    code, edges = spec_edges(spec)
    assert np.array_equal(code.var_chk, ring.var_chk) and np.array_equal(code.chk_deg, ring.chk_deg)
    assert set(code.chk_deg.tolist()) == {4} and set(code.var_deg.tolist()) == {2}
    assert set(forced) <= set(code.var_h.tolist())
    return code, edges, spec


def graph(which, q, poly, method=None):
    """'ring': graph A; 'all': graph B, degree_util.profile_code('all', q, method) (checks 2 .. 8, variables 1 .. 8)"""
    if which == "ring":
        return ring_graph(q, poly)
    from degree_util import profile_code
    return profile_code("all", q, method)


def first_real_frame(N, q):
    """a real-valued, tie-free frame for the non-vacuity assertion"""
    return np.random.default_rng(77 + q).normal(-1.5, 3.0, (N, q - 1))


# ---- OSD: two synthetic shapes of tests/osd_shapes.py rebuilt over another (primitive) modulus -----------------------------------
# (shape, modulus): GF(16) with rows of a CRC-16 generator cut short, and GF(8) with an odd bit length.  The graph and its seed are
# the shape's own; the binary image comes from gf_matrices(q, poly=...), as the loader leaves it (the matrix of x^(q-2) zero) and as
# the full set.  Primitive moduli only: the Mat.Repr layout lists the powers of x.
OSD_CASES = [("crc16_rows5", 25), ("gf8_odd", 13)]
OSD_ORDERS = (0, 1, 2)
OSD_LABELS = ("real",) * 8 + ("weak_last", "integer", "two_valued", "erased")
_OSD = {}


def osd_case(name, poly, as_loaded, exe):
    """One OSD case: the shape's graph, the field's tables and element matrices, 12 frames (eight real-valued ones at
    osd_shapes.EBN0, frame 0 with its last symbol scaled by 0.01, frame 0 rounded to integers, a two-valued frame and frame 2 with
    every third symbol erased) and the CPU checker's answer and counters at orders 0 - 2, computed with THESE matrices.  [CRC rows;
    H_bit] built from them is asserted to be of full row rank.  Cached."""
    import osd_shapes as sh
    from osd_util import run_checker
    key = (name, poly, as_loaded)
    if key not in _OSD:
        code, edges, _, info = sh.shape(name)
        crc_len, crc_rows = sh.crc_of(name)
        f = field(code.q, poly)
        gm = f.gf_mat(as_loaded)
        assert df.is_primitive(code.q, poly) and not np.array_equal(gm, df.gf_matrices(code.q, as_loaded=as_loaded))
        assert np.array_equal(gm[1], np.eye(info["p"], dtype=np.uint8)) and bool(gm[1:].reshape(code.q - 1, -1).any(axis=1).all()) == (not as_loaded)
        assert sh.full_rank(code, crc_len, crc_rows, gf_mat=gm), (name, poly, as_loaded, "[CRC rows; H_bit] is not of full row rank")
        rng = np.random.default_rng(99000 + 10 * poly + as_loaded)
        real = np.concatenate([sh.bpsk_llr_zero(rng, code, 2, e) for e in sh.EBN0], axis=0)
        weak_last = real[0].copy()
        weak_last[-1] *= 0.01
        erased = real[2].copy()
        erased[::3] = 0.0
        L = np.concatenate([real, np.stack([weak_last, np.round(real[0]), np.where(rng.random(real[0].shape) < 0.8, -2.0, 3.0), erased])])
        assert L.shape[0] == len(OSD_LABELS)
        osd = dict(crc_len=crc_len, crc_rows=crc_rows)
        chk = {o: run_checker(exe, code, L, o, 1, gf_mat=gm, counters=True, **osd) for o in OSD_ORDERS}
        _OSD[key] = dict(code=code, edges=edges, info=info, field=f, gf_mat=gm, L=L, chk=chk, osd=osd)
    return _OSD[key]


def osd_oracle_flags(oracle, c, iters):
    """EMS flags, decisions and iteration counts of every frame of an OSD case from the CPU oracle over the case's field"""
    q = c["code"].q
    od = oracle.Decoder(oracle.Code(edges=c["edges"]), c["field"].oracle_gf(oracle), oracle.EMS, iters, oracle.CANONICAL, ems_nm=min(q, 6), ems_nc=2)
    res = [od.decode(L) for L in c["L"]]
    return (np.array([r[0] for r in res], np.uint8), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32))
