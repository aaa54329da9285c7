"""Materialise the text files the drop-in harness reads, in the reference's own formats.

  write_code_file          parity-check file        (parsed by NBLDPC.cpp:147-205 in the reference)
  write_constellation_file "Point: i Real: x Imag: y" (Comm.cpp:113-126)
  write_gf_tables          ./SRC/Arith.Table.GF.<q>.txt and ./SRC/Mat.Repr.GF.<q>.txt (GF.cpp:81-152)

The code and constellation definitions come from nbldpc_amd/data/*.json (imported once from the reference's
data files by tools/import_reference_data.py); the GF tables are GENERATED here from the primitive polynomial.
"""
import functools
import json
import math
import os

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

# primitive polynomials quoted in the first line of the reference's Arith.Table.GF.<q>.txt
PRIMITIVE_POLY = {4: 7, 8: 11, 16: 19, 32: 37, 64: 67, 128: 137, 256: 285, 512: 529}

_codes = None
_cons = None


def codes():
    global _codes
    if _codes is None:
        with open(os.path.join(_DATA, "codes.json")) as f:
            _codes = json.load(f)
    return _codes


def constellations():
    global _cons
    if _cons is None:
        with open(os.path.join(_DATA, "constellations.json")) as f:
            _cons = json.load(f)
    return _cons


def gray_qam(order):
    """Gray-labelled square QAM of `order` = 4^k points at unit average energy, by formula: the first k label bits (the high bits
    of the index, CComm::Modulate is MSB first) choose the in-phase level, the last k the quadrature level; per axis the k bits are
    a Gray code of the level number, level 0 = the most positive amplitude (index 0 -> (+, +), as BPSK's 0 -> +1).
    [(index, re, im)] like constellations()'s entries."""
    k = (order.bit_length() - 1) // 2
    assert order == 4 ** k and k >= 1, order
    n = 1 << k
    amp = {g ^ (g >> 1): float(n - 1 - 2 * g) for g in range(n)}          # Gray code of level g -> amplitude n-1, n-3, .. -(n-1)
    scale = math.sqrt(2.0 * (n * n - 1) / 3.0)                             # sqrt of the mean of re^2 + im^2 over the grid
    return [(i, amp[i >> k] / scale, amp[i & (n - 1)] / scale) for i in range(order)]


# constellations made by formula, beside the ones imported from the reference's data files
GENERATED_CONSTELLATIONS = {"GRAY_QPSK": 4, "GRAY_16QAM": 16}


def constellation(name):
    """[(index, re, im)] of a shipped (constellations()) or generated (GENERATED_CONSTELLATIONS) constellation"""
    if name in GENERATED_CONSTELLATIONS:
        return gray_qam(GENERATED_CONSTELLATIONS[name])
    return constellations()[name]


def code_edges(name):
    """(N, M, q, edge_var, edge_chk, edge_h) with edges in var-major order, 0-based."""
    c = codes()[name]
    ev, ec, eh = [], [], []
    for n, row in enumerate(c["var_rows"]):
        for chk, h in row:
            ev.append(n)
            ec.append(chk - 1)
            eh.append(h)
    return c["N"], c["M"], c["q"], ev, ec, eh


def write_code_file(name, path):
    c = codes()[name]
    lines = [f"{c['N']} {c['M']} {c['q']}", f"{c['maxdv']} {c['maxdc']}",
             " ".join(str(len(r)) for r in c["var_rows"]) + " ",
             " ".join(str(len(r)) for r in c["chk_rows"]) + " "]
    for row in c["var_rows"] + c["chk_rows"]:
        lines.append(" ".join(f"{a} {h}" for a, h in row) + " ")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def write_constellation_file(name, path):
    pts = constellation(name)
    with open(path, "w") as f:
        f.write("\n".join(f"Point:\t{i}\tReal:\t{re!r}\tImag:\t{im!r}" for i, re, im in pts))
    return path


def _mul_x(a, q, poly):
    """a * x modulo `poly` (degree log2(q)), by shift and XOR"""
    a <<= 1
    return a ^ poly if a & q else a


@functools.lru_cache(maxsize=None)
def _irreducible(q):
    p = q.bit_length() - 1
    assert 4 <= q <= 256 and 1 << p == q, q

    def rem(a, d):
        n = d.bit_length()
        while a.bit_length() >= n:
            a ^= d << (a.bit_length() - n)
        return a
    return tuple(f for f in range(q, 2 * q) if all(rem(f, d) for d in range(2, 1 << (p // 2 + 1))))


def irreducible_polys(q):
    """Every irreducible polynomial of degree log2(q) over GF(2) as an integer (bit i = coefficient of x^i), ascending; q <= 256.
    Trial division by every polynomial of degree 1 .. log2(q) / 2, done once per q."""
    return list(_irreducible(q))


def is_primitive(q, poly):
    """True where `poly` is irreducible of degree log2(q) and x generates the multiplicative group of GF(2)[x] / poly."""
    if poly not in _irreducible(q):
        return False
    x, n = 2, 1
    while x != 1:
        x, n = _mul_x(x, q, poly), n + 1
    return n == q - 1


def gf_tables(q, poly=None):
    """(mul[q][q], inv[q]) of GF(q) in the polynomial basis of `poly` (default PRIMITIVE_POLY[q]); add is XOR.  Any irreducible
    polynomial of degree log2(q) gives a field; the Mat.Repr layout of gf_matrices / write_gf_tables needs a primitive one."""
    poly = PRIMITIVE_POLY[q] if poly is None else poly
    p = q.bit_length() - 1
    assert poly >> p == 1, (q, poly)
    mul = [[0] * q for _ in range(q)]
    inv = [0] * q
    for a in range(q):
        for b in range(a, q):
            acc, x = 0, a
            for i in range(p):
                if (b >> i) & 1:
                    acc ^= x
                x <<= 1
                if x & q:
                    x ^= poly
            mul[a][b] = mul[b][a] = acc
            if acc == 1:
                inv[a], inv[b] = b, a
    return mul, inv


def gf_matrices(q, as_loaded=True, poly=None):
    """[q][p][p] uint8: GFElement[e].ValueMatric of every element e, the binary image of "multiply by e" (row i of alpha^k's
    matrix holds the bits of alpha^(k+i), the Mat.Repr.GF.<q>.txt layout).  as_loaded=True: as CGF::Initial leaves them -- it reads
    q-2 of the q-1 non-zero elements (GF.cpp:137), so alpha^(q-2)'s matrix stays zero; False: the full set."""
    import numpy as np
    assert poly is None or is_primitive(q, poly), (q, poly, "the powers of x must reach every non-zero element")
    mul, _ = gf_tables(q, poly)
    p = q.bit_length() - 1
    m = np.zeros((q, p, p), dtype=np.uint8)
    x = 1
    for k in range(q - 2 if as_loaded else q - 1):
        y = x
        for i in range(p):
            m[x, i] = [(y >> j) & 1 for j in range(p)]
            y = mul[y][2]
        x = mul[x][2]
    return m


def write_gf_tables(q, src_dir, poly=None):
    """Write Arith.Table.GF.<q>.txt and Mat.Repr.GF.<q>.txt under src_dir (the reference expects ./SRC/).  With a modulus that
    is irreducible but not primitive the arithmetic table is a field table all the same; the powers of x listed in Mat.Repr then
    repeat before they reach every element, so that file serves OSD only with a primitive modulus."""
    os.makedirs(src_dir, exist_ok=True)
    poly = PRIMITIVE_POLY[q] if poly is None else poly
    mul, inv = gf_tables(q, poly)
    p = q.bit_length() - 1
    with open(os.path.join(src_dir, f"Arith.Table.GF.{q}.txt"), "w") as f:
        f.write(f"GF({q}) with Primitive Polynomial: {poly}. \nMultiply Table:\n")
        for a in range(q):
            f.write(" ".join(map(str, mul[a])) + " \n")
        f.write("Add Table:\n")
        for a in range(q):
            f.write(" ".join(str(a ^ b) for b in range(q)) + " \n")
        f.write("Inverse Table:\n" + " ".join(map(str, inv)) + " \n")
    # companion-matrix powers: row i of A^k holds the coordinates of alpha^(k+i) (alpha = 2)
    with open(os.path.join(src_dir, f"Mat.Repr.GF.{q}.txt"), "w") as f:
        f.write(f"GF({q}) with Primitive Polynomial: {poly} \n")
        x = 1
        for k in range(q - 1):
            f.write(f"A^{k} --> order: {k}\tpoly: {x}\n")
            y = x
            for _ in range(p):
                f.write(" ".join(str((y >> j) & 1) for j in range(p)) + " \n")
                y = mul[y][2]
            x = mul[x][2]
    return src_dir


def materialise(dirpath, q, code_name, constellation_name):
    """Everything one profile needs, laid out like the reference's working directory."""
    os.makedirs(dirpath, exist_ok=True)
    write_gf_tables(q, os.path.join(dirpath, "SRC"))
    write_code_file(code_name, os.path.join(dirpath, code_name + ".txt"))
    write_constellation_file(constellation_name, os.path.join(dirpath, constellation_name + ".txt"))
    return dirpath
