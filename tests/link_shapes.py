"""Synthetic graphs for the link-chain tests: transmitter shapes that no shipped code has.

Every shipped code has q = 16 / 64 / 256, N log2(q) a multiple of 64, rate 1/2, L (received samples per codeword) a multiple of 32
and an encoder without column exchanges.  SHAPES names graphs of tests/degree_util.py::degree_code at the edges of what
nbl_set_transmitter accepts; shape() builds one and ASSERTS the property its line states (N p, (K p - crc_len) % 64, K, L, the
number of column exchanges of the encoder and whether one of them reaches a message column) instead of trusting the table.

A graph is usable when
  * the elimination of CNBLDPC::InitialEncode succeeds (restated here as initial_encode(), which also returns the recorded column
    exchanges), and
  * the compiled reference can initialise it: its CNBLDPC::Initial builds the OSD matrices whatever the decode method is and never
    ends on a bit-level H that is not of full row rank (tests/osd_shapes.py::full_rank), and its CRC generator needs crcLen 8, 16 or
    24 (with crcLen 0 its elimination runs on an all-zero matrix and never ends: `k1` is the one shape without a fixture from the
    reference's chain, see NO_REFERENCE).
`python tests/link_shapes.py [id ...]` tries the seeds of SEEDS in turn and prints, per shape, the first one that meets the shape's
conditions; that seed is written into the table below.
"""
import functools

import numpy as np

from degree_util import degree_code

SEEDS = range(9300, 13300)

# id -> q, M, check-degree cycle, variable-degree cycle, seed, crc_len, nqam (2 or q; default 2), punct (degree whose variables are
# punctured, default 0 = none), poly (the modulus the GF tables of the work directory and of the decoder are made from, default: the
# one of nbldpc_amd/datafiles.py::PRIMITIVE_POLY) and `expect`: the properties the shape is in the table for.  exch = number of column exchanges of the
# encoder, exch_msg / exch_parity = how many of them reach a column below K (then gen[:K] is not the identity) / at or above K.
SHAPES = {
    # GF(4), N p < 64: one partial wave of encode rows, nw = 1, L < 64.  The smallest shape: lane strides and the encode chunks run on it
    "one_word": dict(q=4, M=16, chk=(4, 5), var=(2, 2, 3), seed=9300, crc_len=8, expect=dict(N=31, Np=62, nw=1, L=62)),
    # GF(8): N p and L odd, K p - crc_len = 193 = 3 * 64 + 1 with CRC-8 (3 K = 9 + 64 k has K = 3, 67, 131 ..: word 3 holds one bit)
    "gf8_odd": dict(q=8, M=34, chk=(6,), var=(2,) * 49 + (3,), seed=9300, crc_len=8, expect=dict(K=67, Np_odd=1, L_odd=1, nb_mod64=1)),
    # GF(32): K p - crc_len = 319 = 4 * 64 + 63 with CRC-16 (the smallest K with 5 K = 79 + 64 k)
    "gf32_63": dict(q=32, M=34, chk=(6,), var=(2,) * 49 + (3,), seed=9300, crc_len=16, expect=dict(K=67, nb_mod64=63)),
    # GF(128): CRC-24 with K p = 28 just above 24, K < 64
    "gf128_crc24": dict(q=128, M=8, chk=(3,), var=(2,), seed=9300, crc_len=24, expect=dict(K=4, nb=4)),
    # K = 1: one message symbol, the one-wave reduction of the error count with 63 idle lanes.  crc_len 0 (CRC-8 does not fit
    # below GF(256), where it fills the message)
    "k1": dict(q=16, M=12, chk=(2, 2, 2, 2, 2, 3), var=(2,), seed=9300, crc_len=0, expect=dict(K=1, nb=4)),
    # K = 65: the second trip of the error-count loop holds one symbol
    "k65": dict(q=4, M=65, chk=(4,), var=(2,), seed=9301, crc_len=8, expect=dict(K=65)),
    # N p = 258: the second block of encode rows holds two rows (257 is prime: no N p equals it; 258 = 129 * 2 is the smallest above 256)
    "rows_258": dict(q=4, M=43, chk=(6,), var=(2,), seed=9300, crc_len=8, expect=dict(N=129, Np=258)),
    # the elimination exchanges a message column: gen[:K] is not the identity, the slot's message is not the PN draw
    "exchange_msg": dict(q=16, M=12, chk=(4,), var=(2,), seed=9300, crc_len=8, expect=dict(N=24, exch_msg_min=1)),
    "exchange_msg_crc24": dict(q=16, M=12, chk=(4,), var=(2,), seed=9300, crc_len=24, expect=dict(N=24, exch_msg_min=1)),
    # an exchange between two parity columns.  (Exchanges among parity columns ONLY do not exist: a column is exchanged at row r when
    # it is zero in rows 0 .. r, and moved to the pivot position of a row above it stays zero there, so that row exchanges it again;
    # every chain of exchanges ends in a message column.  This shape has a chain that passes through a parity column.)
    "exchange_chain": dict(q=16, M=12, chk=(4,), var=(2,), seed=9310, crc_len=8, expect=dict(N=24, exch_parity_min=1, exch_msg_min=1)),
    # crc_len == K p: no PN bit at all, the all-zero branch of the transmit path with random_msg = 1
    "crc_fills_message": dict(q=16, M=8, chk=(2, 3), var=(2,), seed=9300, crc_len=8, expect=dict(K=2, nb=0)),
    # M = N / 8 and K = N / 8
    "high_rate": dict(q=16, M=8, chk=(8,), var=(1,), seed=9300, crc_len=8, expect=dict(N=64, K=56, Np=256)),
    "low_rate": dict(q=16, M=56, chk=(3,), var=(3, 3, 2, 3, 3, 2, 3, 2), seed=9300, crc_len=8, expect=dict(N=64, K=8, Np=256)),
    # one constellation point per code symbol, q = 4 .. 128
    "qary_gf4": dict(q=4, M=16, chk=(4, 5), var=(2, 2, 3), seed=9300, crc_len=8, nqam=4, expect=dict(N=31, L=31)),
    # .. with punctured symbols (the degree-3 variables): src[n] = -1 in the demodulator, whole symbols skipped by the modulator
    "qary_gf8_punct": dict(q=8, M=12, chk=(4, 5), var=(2,) * 5 + (3,), seed=9478, crc_len=8, nqam=8, punct=3,
                           expect=dict(punct_min=3, punct_alone=1)),
    "qary_gf16": dict(q=16, M=12, chk=(4,), var=(2,), seed=9300, crc_len=16, nqam=16, expect=dict(N=24, L=24)),
    "qary_gf32": dict(q=32, M=10, chk=(4,), var=(2,), seed=9300, crc_len=8, nqam=32, expect=dict(N=20, L=20)),
    "qary_gf128": dict(q=128, M=8, chk=(3,), var=(2,), seed=9300, crc_len=8, nqam=128, expect=dict(N=12, L=12)),
    # BPSK with punctured symbols 0, N - 1 and two adjacent ones (the degree-3 variables)
    "punct_ends": dict(q=16, M=10, chk=(4, 5), var=(2, 2, 2, 3), seed=9321, crc_len=8, punct=3, expect=dict(punct_ends=1)),
    # another field representation: tables, generator matrix and the reference's own chain all made with a primitive polynomial that
    # is not the default one (19 -> 25, 67 -> 91), BPSK and one point per symbol.  The GF(16) graph's encoder exchanges a message
    # column, so gen[:K] holds products of the alternative table
    "gf16_m25": dict(q=16, M=12, chk=(4,), var=(2,), seed=9300, crc_len=8, poly=25, expect=dict(N=24, exch_msg_min=1)),
    "qary_gf64_m91": dict(q=64, M=8, chk=(3,), var=(2,), seed=9300, crc_len=8, nqam=64, poly=91, expect=dict(N=12, L=12)),
}
FIELD_SHAPES = ("gf16_m25", "qary_gf64_m91")
# shapes the compiled reference cannot run (module docstring): the host chain is held to the reference on every other shape, and on
# these the GPU tests compare with the host chain alone
NO_REFERENCE = ("k1",)
# the lane-stride cases run on this shape
SMALLEST = "one_word"
# shapes with a FER anchor row of the compiled reference (tests/golden/fer_anchors_link.json)
FER_SHAPES = ("exchange_msg", "qary_gf8_punct", "gf8_odd")


@functools.lru_cache(maxsize=None)
def pn_period():
    """Period of the PN register, by clocking the host chain's GenPN from lane 0's initial contents until they come back."""
    from nbldpc_amd import hostlib
    s0 = hostlib.pn_initial(0)
    s, n = hostlib.pn_clock(s0, 1), 1
    while s != s0:
        s, n = hostlib.pn_clock(s, 1), n + 1
        assert n <= 4096, "the register does not return to its initial contents"
    return n


def stride_cases():
    """tag -> `parallel` of the lane-stride cases: the PN stride one below, at, one above and at twice the register's period (the
    transmit kernel works with parallel % period: 0 gives every message bit of a lane the same value, above the period it wraps)"""
    T = pn_period()
    return {"period_minus_1": T - 1, "period": T, "period_plus_1": T + 1, "twice_period": 2 * T}


@functools.lru_cache(maxsize=None)
def gf_np(q, poly=None):
    import nbldpc_amd.datafiles as df
    mul, inv = df.gf_tables(q, poly)
    return np.array(mul, dtype=np.int64), np.array(inv, dtype=np.int64)


def initial_encode(spec, poly=None):
    """CNBLDPC::InitialEncode restated: Gauss elimination from the last row up with the pivot of row r in column r + K; a missing
    pivot is fetched from a row above, else from the nearest column to the left that has an entry in this row (the exchange is
    recorded).  Returns the recorded exchanges [(col, left), ..] in the order they were made, or None where no pivot is found."""
    N, M, q = spec["N"], spec["M"], spec["q"]
    mul, inv = gf_np(q, poly)
    H = np.zeros((M, N), dtype=np.int64)
    for m, row in enumerate(spec["chk_rows"]):
        for v, h in row:
            H[m, v - 1] = h
    swaps = []
    for row in range(M - 1, -1, -1):
        col = row + N - M
        if H[row, col] == 0:
            up = next((u for u in range(row - 1, -1, -1) if H[u, col]), None)
            if up is not None:
                H[[row, up]] = H[[up, row]]
            else:
                left = next((c for c in range(col - 1, -1, -1) if H[row, c]), None)
                if left is None:
                    return None
                H[:, [col, left]] = H[:, [left, col]]
                swaps.append((col, left))
        hinv = inv[H[row, col]]
        for up in range(row - 1, -1, -1):
            if H[up, col]:
                H[up] ^= mul[mul[hinv, H[up, col]], H[row]]
        H[row, :col + 1] = mul[hinv, H[row, :col + 1]]
    return swaps


def grid_points(q):
    """The q points of a rectangular grid, 2^ceil(p/2) columns by 2^floor(p/2) rows, point i in column i % columns, scaled to unit
    mean energy: the constellation of the q-ary shapes.  Distinct points, no Gray labelling: only data for the chain under test."""
    p = q.bit_length() - 1
    cols, rows = 1 << ((p + 1) // 2), 1 << (p // 2)
    i = np.arange(q)
    pts = np.stack([2.0 * (i % cols) - (cols - 1), 2.0 * (i // cols) - (rows - 1)], axis=1)
    pts /= np.sqrt((pts ** 2).sum(axis=1).mean())
    assert len({tuple(x) for x in pts.tolist()}) == q
    return pts


def build(name, seed):
    s = SHAPES[name]
    return degree_code(s["q"], seed, s["chk"], s["var"], s["M"])


def describe(name, code, spec):
    """Geometry of a shape as CComm::Initial derives it, and the exchanges of its encoder (None: the elimination fails)."""
    s = SHAPES[name]
    q, N, M = s["q"], code.N, code.M
    p, K = q.bit_length() - 1, code.N - code.M
    order = s.get("nqam", 2)
    punct = [n for n in range(N) if s.get("punct", 0) and int(code.var_deg[n]) == s["punct"]]
    mb = order.bit_length() - 1
    nb = K * p - s["crc_len"]
    swaps = initial_encode(spec, s.get("poly"))
    # no check holds two punctured variables: every punctured symbol (channel LLR 0) has a check that determines it
    alone = all(sum(v - 1 in punct for v, _ in row) <= 1 for row in spec["chk_rows"])
    return dict(punct_alone=int(alone), q=q, N=N, M=M, K=K, p=p, Np=N * p, nb=nb, nw=(nb + 63) // 64, crc_len=s["crc_len"], order=order, punct=punct,
                L=(N - len(punct)) * p // mb, swaps=swaps)


def meets(name, info):
    """The properties of the table line, as a dict of (got, want)."""
    N, K, punct, swaps = info["N"], info["K"], info["punct"], info["swaps"] or []
    adjacent = any(b - a == 1 for a, b in zip(punct, punct[1:]))
    got = dict(N=N, K=K, Np=info["Np"], Np_odd=info["Np"] % 2, L=info["L"], L_odd=info["L"] % 2, nb=info["nb"], nb_mod64=info["nb"] % 64,
               nw=info["nw"], exch=len(swaps), exch_msg=sum(left < K for _, left in swaps), exch_parity=sum(left >= K for _, left in swaps),
               punct_alone=info["punct_alone"], punct_ends=int(bool(punct) and punct[0] == 0 and punct[-1] == N - 1 and adjacent))
    out = {}
    for key, want in SHAPES[name]["expect"].items():
        if key.endswith("_min"):
            base = key[:-4]
            val = len(punct) if base == "punct" else got[base]
            out[key] = (val, want, val >= want)
        else:
            out[key] = (got[key], want, got[key] == want)
    return out


def reference_can_initialise(code, poly=None):
    import nbldpc_amd.datafiles as df
    from osd_shapes import full_rank
    return full_rank(code, 8, 0, gf_mat=None if poly is None else df.gf_matrices(code.q, poly=poly))


@functools.lru_cache(maxsize=None)
def shape(name):
    """(nb.Code, spec, info) of a named shape; info: q, N, M, K, p, Np, nb, nw, crc_len, order, punct, L, swaps.  The properties the
    table states are asserted, and so are the two conditions of the module docstring."""
    s = SHAPES[name]
    code, _, spec = build(name, s["seed"])
    info = describe(name, code, spec)
    assert info["swaps"] is not None, (name, "the elimination of InitialEncode finds no pivot")
    for key, (got, want, ok) in meets(name, info).items():
        assert ok, (name, key, got, want)
    assert info["K"] >= 1 and 0 <= info["nb"] and info["order"] in (2, s["q"]), (name, info)
    assert reference_can_initialise(code, s.get("poly")), (name, "bit-level H is not of full row rank")
    return code, spec, info


def poly_of(name):
    """the modulus of a shape's field, None for the default one"""
    return SHAPES[name].get("poly")


def profile_of(name, parallel, **over):
    """Profile keys of a shape (nbldpc_amd/profiles.py), without the code and constellation file names: EMS, five iterations."""
    s = SHAPES[name]
    q = s["q"]
    kw = dict(gfq=q, method=2, max_iter=5, ems_nm=min(q, 8), ems_nc=2, crc_len=s["crc_len"], nqam=s.get("nqam", 2),
              puncture_degree=s.get("punct", 0), random_msg=1, parallel=parallel)
    kw.update(over)
    return kw


def points_of(name):
    """Constellation points [order][2] of a shape: BPSK as shipped, the grid for the q-ary shapes."""
    import nbldpc_amd.datafiles as df
    s = SHAPES[name]
    if s.get("nqam", 2) == 2:
        return np.array([[x[1], x[2]] for x in sorted(df.constellations()["BPSK"])], dtype=np.float64)
    return grid_points(s["q"])


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in sys.argv[1:] or list(SHAPES):
        found = None
        for seed in SEEDS:
            try:
                code, _, spec = build(name, seed)
            except AssertionError as e:
                print(name, seed, "no graph:", e)
                break
            info = describe(name, code, spec)
            if info["swaps"] is None or not all(ok for _, _, ok in meets(name, info).values()) or not reference_can_initialise(code, SHAPES[name].get("poly")):
                continue
            found = seed
            break
        print(f"{name}: seed={found} N={code.N} K={code.N - code.M} Np={info['Np']} nb={info['nb']} L={info['L']} "
              f"punct={info['punct']} swaps={info['swaps']}", flush=True)
