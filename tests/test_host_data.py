"""Host-side data: GF tables generated from the primitive polynomial, code / constellation file writers."""
import json
import os

import numpy as np
import pytest

import nbldpc_amd.datafiles as df
from conftest import GOLD, token_digest, value_digest
from nbldpc_amd.shard import shard_range, shard_sizes

# digests of the reference's own data files (tests/golden/make_golden.py data)
REF = json.load(open(os.path.join(GOLD, "reference_data.json")))


@pytest.mark.parametrize("q", [4, 8, 16, 32, 64, 128, 256])
def test_gf_field_axioms(q):
    mul, inv = df.gf_tables(q)
    mul = np.array(mul)
    assert np.array_equal(mul, mul.T) and np.all(mul[0] == 0) and np.array_equal(mul[1], np.arange(q))
    for a in range(1, q):
        assert mul[a, inv[a]] == 1
        assert sorted(mul[a, 1:]) == list(range(1, q))  # multiplication by a is a permutation
    a, b, c = np.meshgrid(np.arange(q), np.arange(min(q, 16)), np.arange(min(q, 16)), indexing="ij")
    assert np.array_equal(mul[a, b ^ c], mul[a, b] ^ mul[a, c])  # distributive over XOR
    # alpha = 2 is primitive
    x, seen = 1, set()
    for _ in range(q - 1):
        seen.add(x)
        x = mul[x, 2]
    assert len(seen) == q - 1 and x == 1


def test_irreducible_and_primitive_polynomial_counts():
    """Degree 2 .. 8: (2^p necklace counts) 1, 2, 3, 6, 9, 18, 30 irreducible polynomials, phi(2^p - 1) / p = 1, 2, 2, 6, 6, 18, 16
    primitive ones; the default of every q is among the primitive ones."""
    qs = (4, 8, 16, 32, 64, 128, 256)
    irr = {q: df.irreducible_polys(q) for q in qs}
    assert [len(irr[q]) for q in qs] == [1, 2, 3, 6, 9, 18, 30]
    assert [sum(df.is_primitive(q, f) for f in irr[q]) for q in qs] == [1, 2, 2, 6, 6, 18, 16]
    for q in qs:
        assert irr[q] == sorted(irr[q]) and all(q <= f < 2 * q and f & 1 for f in irr[q])
        assert df.is_primitive(q, df.PRIMITIVE_POLY[q])
        assert not df.is_primitive(q, q | 1 if (q | 1) not in irr[q] else q)      # a reducible polynomial is not primitive
    assert not df.is_primitive(16, 31) and 31 in irr[16] and not df.is_primitive(256, 283) and 283 in irr[256]
    assert 21 not in irr[16]                                                      # (x^2 + x + 1)^2


@pytest.mark.parametrize("q", [4, 8, 16, 32, 64, 128, 256])
def test_every_irreducible_modulus_gives_a_field(q):
    """gf_tables(q, poly) for EVERY irreducible polynomial of degree log2(q): commutative, mul[a][inv[a]] == 1, distributive over
    XOR, x * a the shift-and-XOR product.  Exhaustive for q <= 64; at q = 128 / 256 rows 1, 2, 3, q / 2, q - 1 exhaustively and a
    seeded sample of rows."""
    rng = np.random.default_rng(q)
    for poly in df.irreducible_polys(q):
        mul, inv = df.gf_tables(q, poly)
        mul, inv = np.array(mul), np.array(inv)
        assert np.array_equal(mul, mul.T) and not mul[0].any() and np.array_equal(mul[1], np.arange(q)), poly
        assert np.array_equal(mul[np.arange(1, q), inv[1:]], np.ones(q - 1, dtype=mul.dtype)), poly
        assert (q | mul[2, q // 2]) == poly
        sh = np.arange(q) << 1
        assert np.array_equal(mul[2], np.where(sh & q, sh ^ poly, sh)), poly
        rows = np.arange(q) if q <= 64 else np.unique(np.concatenate([[1, 2, 3, q // 2, q - 1], rng.integers(1, q, 12)]))
        b, c = np.meshgrid(np.arange(q), np.arange(q), indexing="ij")
        for a in rows:
            assert np.array_equal(mul[a][b ^ c], mul[a][b] ^ mul[a][c]), (poly, int(a))   # distributive over XOR
            assert sorted(mul[a, 1:]) == list(range(1, q)) or a == 0, (poly, int(a))      # no zero divisors
        if q <= 64:                                                                       # associative
            a3 = rng.integers(0, q, (3, 4096))
            assert np.array_equal(mul[mul[a3[0], a3[1]], a3[2]], mul[a3[0], mul[a3[1], a3[2]]]), poly
    assert df.gf_tables(q) == df.gf_tables(q, df.PRIMITIVE_POLY[q])


def test_table_files_of_another_modulus(tmp_path, oracle):
    """write_gf_tables(q, dir, poly): the oracle's loader reads back the tables of that modulus and names it; the default output is
    the same with and without the argument."""
    df.write_gf_tables(16, str(tmp_path / "a"))
    df.write_gf_tables(16, str(tmp_path / "b"), df.PRIMITIVE_POLY[16])
    df.write_gf_tables(16, str(tmp_path / "c"), 25)
    for f in ("Arith.Table.GF.16.txt", "Mat.Repr.GF.16.txt"):
        assert open(tmp_path / "a" / f, "rb").read() == open(tmp_path / "b" / f, "rb").read()
        assert open(tmp_path / "a" / f, "rb").read() != open(tmp_path / "c" / f, "rb").read()
    g = oracle.GF(16, arith_path=str(tmp_path / "c" / "Arith.Table.GF.16.txt"))
    mul, inv = df.gf_tables(16, 25)
    assert np.array_equal(g.mul, np.array(mul)) and np.array_equal(g.inv[1:], np.array(inv)[1:]) and g.s.poly == 25
    assert oracle.GF(16, arith_path=str(tmp_path / "a" / "Arith.Table.GF.16.txt")).s.poly == 19
    m = df.gf_matrices(16, as_loaded=False, poly=25)
    assert np.array_equal(m[1], np.eye(4, dtype=np.uint8)) and all(m[e].any() for e in range(1, 16))
    assert np.array_equal(df.gf_matrices(16), df.gf_matrices(16, poly=19))


def test_oracle_gf_equals_python(oracle):
    for q in (16, 64, 256):
        mul, inv = df.gf_tables(q)
        g = oracle.GF(q)
        assert np.array_equal(g.mul, np.array(mul)) and np.array_equal(g.inv[1:], np.array(inv)[1:])


@pytest.mark.parametrize("q", [4, 8, 16, 32, 64, 128, 256, 512])
def test_generated_tables_equal_reference_files(tmp_path, q):
    df.write_gf_tables(q, str(tmp_path))
    for stem in ("Arith.Table.GF", "Mat.Repr.GF"):
        f = f"{stem}.{q}.txt"
        assert token_digest(open(tmp_path / f).read().split()) == REF["tokens"][f], f


def test_code_and_constellation_files_equal_reference(tmp_path):
    assert sorted(n + ".txt" for n in df.codes()) == sorted(f for f in REF["tokens"] if not f.startswith(("Arith.", "Mat.")))
    for name in df.codes():
        p = df.write_code_file(name, str(tmp_path / (name + ".txt")))
        assert token_digest(open(p).read().split()) == REF["tokens"][name + ".txt"], name
    assert sorted(n + ".txt" for n in df.constellations()) == sorted(REF["values"])
    for name in df.constellations():
        p = df.write_constellation_file(name, str(tmp_path / (name + ".txt")))
        assert value_digest(open(p).read().split()) == REF["values"][name + ".txt"], name


def test_code_file_roundtrip_through_oracle_loader(tmp_path, oracle):
    for name, c in df.codes().items():
        p = df.write_code_file(name, str(tmp_path / "c.txt"))
        code = oracle.Code(path=p)
        N, M, q, ev, ec, eh = df.code_edges(name)
        assert (code.N, code.M, code.q, code.E) == (N, M, q, len(ev))
        v, ch, h = code.edge_list()
        assert list(v) == ev and list(ch) == ec and list(h) == eh
        # every check row lists its variables in increasing order in the shipped files (relied on by from_edges)
        for row in c["chk_rows"]:
            vs = [x[0] for x in row]
            assert vs == sorted(vs)


def test_shard_ranges_cover_batch():
    for B in (0, 1, 7, 8, 16384, 16385):
        for W in (1, 2, 3, 8):
            rs = [shard_range(B, r, W) for r in range(W)]
            assert rs[0][0] == 0 and rs[-1][1] == B
            assert all(rs[i][1] == rs[i + 1][0] for i in range(W - 1))
            assert max(shard_sizes(B, W)) - min(shard_sizes(B, W)) <= 1
