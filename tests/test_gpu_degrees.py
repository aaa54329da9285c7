"""Every node degree the C ABI accepts (checks 2-8, variables 1-8) on a real MI355X, all kernel families against the CPU restatements.

The shipped codes have checks of degree 4 / 5 and variables of degree 2; tests/degree_util.py builds small graphs for six degree
profiles (dc2, dc2mix, dc78, dv48, dv4edge, all) and every cell of profile x field x method runs here in the three kernel variants
of nbl_debug_force_generic: message state, decisions, flags and iteration counts against the canonical oracle (EMS / T-EMS: bit
for bit; integer frames also against the literal restatement), the BS-TEMS checker (bit for bit) or within 1e-9 (log-QSPA).  The
oracle itself is pinned to the compiled reference at these degrees by the deg_* fixtures (tests/test_oracle_golden.py), which
the kernels reproduce here as well."""
import numpy as np
import pytest

import nbldpc_amd as nb
from conftest import load_golden, decoder_kwargs
from bstems_util import CANONICAL as BS_CANONICAL, LITERAL as BS_LITERAL, bs_kwargs, build_checker, run_checker
from degree_util import PROFILES, QS, TEMS_REFUSED, degree_code, profile_code, ring_code, spec_edges
from nbldpc_amd.binding import debug_plan
from test_gpu_parity import LLR_TOL, _bpsk_llr_zero, _force_generic

pytestmark = pytest.mark.gpu

METHODS = ("ems", "ems_plain", "tems", "bp", "bstems")
CELLS = [(prof, q, m) for prof in PROFILES for q in QS for m in METHODS if not (m == "tems" and (prof, q) in TEMS_REFUSED)]
BS_NM = {4: 3, 8: 4, 16: 6, 32: 7, 64: 8, 128: 10, 256: 12}   # < q and <= 16; below, at and above log2(q)
DEG_FIXTURES = ["deg_all_gf16_ems", "deg_all_gf16_tems", "deg_all_gf16_bp", "deg_all_gf16_bstems", "deg_dc78_gf64_ems",
                "deg_dv48_gf4_tems", "deg_dc2_gf256_bp"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("bstems_deg"))


def method_runs(method, q):
    """[(ABI method, shaped parameters, plain parameters)] of one method id: the shaped set (factor / offset dead zone) goes with
    real-valued frames, the plain one (factor 1, offset 0: exact arithmetic) with integer frames."""
    if method in ("ems", "ems_plain"):
        nc = 2 if method == "ems" else 7                # layered deviation counting | nc >= maxdc - 1: plain convolution
        return [(nb.METHOD_EMS, dict(ems_nm=nm, ems_nc=nc, ems_factor=1.15, ems_offset=0.2), dict(ems_nm=nm, ems_nc=nc, ems_factor=1.0, ems_offset=0.0))
                for nm in ((8, 16) if q == 256 else (min(q, 6),))]
    if method == "tems":
        nc = 3 if q <= 64 else 2
        return [(nb.METHOD_TEMS, dict(tems_nr=2, tems_nc=nc, tems_factor=1.1, tems_offset=0.15), dict(tems_nr=2, tems_nc=nc, tems_factor=1.0, tems_offset=0.0))]
    if method == "bstems":
        return [(nb.METHOD_BS_TEMS, dict(bs_nm=BS_NM[q], bs_nc=2, bs_factor=1.25, bs_offset=0.1), dict(bs_nm=BS_NM[q], bs_nc=2, bs_factor=1.0, bs_offset=0.0))]
    return [(nb.METHOD_BP, dict(), dict())]


def literal_affordable(meth, kw, maxdc):
    """The literal EMS restatement enumerates, like the reference, up to nm ^ min(nc, maxdc - 1) configurations per output edge:
    16 ^ 7 at (nm 16, plain convolution, check degree 8) -- eight minutes on one core for one 12-check graph (measured), against
    four seconds for nm = 8 (8 ^ 7), which runs.  Beyond 2 ^ 21 configurations the integer frames are compared with the canonical
    restatement alone; in this grid that is GF(256), nm = 16, nc = 7 on dc78 and all."""
    if meth == nb.METHOD_BS_TEMS:
        return False  # (ties: test_degree_grid_vs_oracle says why, and what runs in its place)
    return meth != nb.METHOD_EMS or kw["ems_nm"] ** min(kw["ems_nc"], maxdc - 1) <= 1 << 21


def real_frames(rng, N, q):
    L = rng.normal(-1.5, 3.0, (3, N, q - 1))
    L[1, ::3] = 0.0                                     # every third symbol erased
    L[2] = 0.0                                          # everything ties
    return L


def integer_frames(rng, N, q):
    L = np.round(rng.normal(-1, 2, (2, N, q - 1)))      # tie-heavy
    L[1] = np.where(rng.random((N, q - 1)) < 0.8, -2.0, 3.0)  # two-valued
    return L


def bp_frames(rng, N, q):
    L = rng.normal(-1.5, 3.0, (4, N, q - 1))
    L[1] = rng.normal(-0.5, 1.0, (N, q - 1))
    L[2] = 0.0
    L[3] = rng.normal(-800, 600, (N, q - 1))            # LLRs hundreds of nats apart
    return L


def reference(oracle, checker, code, edges, meth, iters, L, kw, mode, fixed=0, gf=None):
    """[(flag, decisions, iterations, (post, v2c, c2v))] per frame: BS-TEMS from tests/bstems_check.cpp, the rest from the oracle.
    mode: 'canonical' | 'literal'.  gf: a tests/field_util.py::Field (its tables for the checker, its loaded table file for the
    oracle); None: the field of the default polynomial."""
    if meth == nb.METHOD_BS_TEMS:
        out, ret, its, st = run_checker(checker, code, L, iters, BS_CANONICAL if mode == "canonical" else BS_LITERAL, fixed_iters=fixed,
                                        state=range(L.shape[0]), gf=None if gf is None else gf.tables, **kw)
        return [(int(ret[b]), out[b].copy(), int(its[b]), st[b]) for b in range(L.shape[0])]
    od = oracle.Decoder(oracle.Code(edges=edges), oracle.GF(code.q) if gf is None else gf.oracle_gf(oracle), meth, iters, oracle.CANONICAL if mode == "canonical" else oracle.LITERAL,
                        fixed_iters=fixed, **kw)
    ref = []
    for b in range(L.shape[0]):
        r, o, it = od.decode(L[b])
        ref.append((r, o.copy(), it, [x.copy() for x in od.state()]))
    return ref


def gpu_equals(code, meth, iters, L, kw, refs, exact, tag, variants=(0, 1, 2), fixed=0, gf=None):
    """Decode L in every kernel variant; decisions, flags, iteration counts and the message state of every frame against each
    reference in `refs`.  (v2c of a codeword that converged at iteration k >= 2 is not compared unless iterations are fixed:
    include/nbldpc.h, nbl_read_state -- the variable-node pass has already written iteration k's messages.)
    gf: the Field whose tables nbl_create gets (None: the default polynomial's)."""
    for variant in variants:
        dec = nb.Decoder(code, meth, iters, fixed_iters=fixed, gf=None if gf is None else gf.tables, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        out, conv, its = dec.decode(L)
        for ri, ref in enumerate(refs):
            for b in range(L.shape[0]):
                r, o, it, st = ref[b]
                assert (conv[b], its[b]) == (r, it) and np.array_equal(out[b], o), (tag, variant, ri, b)
                for k, (a, x) in enumerate(zip(dec.read_state(b), st)):
                    if k == 1 and r == 1 and it >= 2 and not fixed:
                        continue
                    if exact:
                        assert np.array_equal(a, x), (tag, variant, ri, b, "post v2c c2v".split()[k])
                    else:
                        assert np.all(np.isfinite(a)), (tag, variant, b)
                        assert np.max(np.abs(a - x)) <= LLR_TOL * max(1.0, np.max(np.abs(x))), (tag, variant, ri, b, "post v2c c2v".split()[k])
        dec.close()


@pytest.mark.parametrize("profile,q,method", CELLS, ids=[f"{p}-gf{q}-{m}" for p, q, m in CELLS])
def test_degree_grid_vs_oracle(oracle, checker, profile, q, method):
    """One (profile, field, method) cell, three iterations, kernel variants 0 / 1 / 2.
      * EMS (layered nc = 2, plain nc = 7), T-EMS, BS-TEMS: shaped real-valued frames (one with every third symbol erased, one
        all-zero) bit for bit against the canonical restatement; integer frames (tie-heavy, two-valued) with factor 1 / offset 0
        against the canonical AND the literal one (every sum exact, the reference's residue vanishes; literal_affordable names
        the two cells where the literal enumeration is out of reach).  Integer inputs are never
        combined with a factor like 1.1 (test_gpu_parity.py::test_tems_gf64_every_shape_ties_and_erasures_vs_oracle says why).
      * log-QSPA: ordinary, narrow, all-zero frames and one with LLRs hundreds of nats apart; decisions, flags and iteration
        counts equal, state within 1e-9 of the oracle's FP64 restatement.  Left out for log-QSPA, as in test_gpu_parity.py: frames
        with some symbols erased (a check with two erased edges sends LLRs that are zero up to rounding noise, whose sign then
        decides an erased variable and the damping), integer frames (exact ties between symbols, broken by the last bit of an
        exp/log chain), and more than 3 iterations (these graphs are full of 4-cycles; a variable's own L_ch comes back with the
        opposite sign and leaves v2c entries that are zero up to rounding noise).  dc78 runs 2 iterations: twelve checks of degree
        7 / 8 over 36 variables share several variables pairwise, and the echo is there at iteration 3 already -- measured at
        GF(4) on the wide frame: an a-posteriori LLR of 5.7e-14 in the small-field kernels against 0.0 exactly in the oracle and
        the general kernel (state within 5e-16 of each other everywhere), and the hard decision is the sign of that.
    The T-EMS cells of TEMS_REFUSED (log2(q) * maxdc > 32) do not exist; tests/test_abi.py asserts that nbl_create refuses exactly
    those.  At GF(128) / GF(256) the T-EMS cell of dv48 has checks of degree 3 / 4 (degree_util.TEMS_CHK_DEGS)."""
    code, edges, _ = profile_code(profile, q, method)
    rng = np.random.default_rng(1000 * q + 7 * sorted(PROFILES).index(profile) + METHODS.index(method))
    for meth, shaped, plain in method_runs(method, q):
        tag = (profile, q, method, tuple(shaped.values())[:1])
        if method == "bp":
            L = bp_frames(rng, code.N, q)
            iters = 2 if profile == "dc78" else 3
            gpu_equals(code, meth, iters, L, {}, [reference(oracle, checker, code, edges, meth, iters, L, {}, "canonical")], False, tag)
            continue
        L = real_frames(rng, code.N, q)
        gpu_equals(code, meth, 3, L, shaped, [reference(oracle, checker, code, edges, meth, 3, L, shaped, "canonical")], True, tag)
        if meth == nb.METHOD_BS_TEMS:
            # the literal BS-TEMS restatement orders the symbols of a check with std::sort on the value alone, as the reference
            # does: among EQUAL values the order is whatever that sort leaves (and changes with the array length), so frames with
            # ties have no literal answer to compare with.  Its tie-free frame runs instead: decisions, flags, iteration counts
            # equal, state within 1e-9 (the running-sum residue), factor 1 / offset 0; integer frames against the canonical one.
            gpu_equals(code, meth, 3, L[:1], plain, [reference(oracle, checker, code, edges, meth, 3, L[:1], plain, "literal")], False, tag)
        L = integer_frames(rng, code.N, q)
        modes = ("canonical", "literal") if literal_affordable(meth, plain, int(code.chk_deg.max())) else ("canonical",)
        gpu_equals(code, meth, 3, L, plain, [reference(oracle, checker, code, edges, meth, 3, L, plain, m) for m in modes], True, tag)


@pytest.mark.parametrize("profile,q", [("dc78", 16), ("all", 16), ("dc78", 8), ("all", 4), ("dv4edge", 32), ("dv48", 64)])
def test_tems_nc4_general_kernel_up_to_the_32_bit_path_code(oracle, checker, profile, q):
    """tems_nc = 4 is beyond the small-field and the nc <= 3 general kernel (the grid's tems_nc is 2 / 3), so every variant runs
    cn_tems_kernel, the kernel for any nc: path codes of exactly 32 bits (GF(16) with checks of degree 8: the first column's digit sits at
    bit 28 and the word is full), 30 bits (GF(64), degree 5), 24, 20 and 16 bits.  (GF(256), degree 4, is
    32 bits too, but the oracle's T-EMS with nc = 4 takes 200 s for one 12-check graph there; GF(256) runs in the grid with nc = 2.)
    Shaped real-valued frames against the canonical oracle, integer frames against the canonical and the literal one."""
    code, edges, _ = profile_code(profile, q, "tems")
    assert (q.bit_length() - 1) * int(code.chk_deg.max()) == {("dc78", 16): 32, ("all", 16): 32, ("dc78", 8): 24, ("all", 4): 16,
                                                               ("dv4edge", 32): 20, ("dv48", 64): 30}[(profile, q)]
    rng = np.random.default_rng(4000 + q + len(profile))
    shaped = dict(tems_nr=2, tems_nc=4, tems_factor=1.1, tems_offset=0.15)
    plain = dict(tems_nr=2, tems_nc=4, tems_factor=1.0, tems_offset=0.0)
    L = real_frames(rng, code.N, q)
    gpu_equals(code, nb.METHOD_TEMS, 3, L, shaped, [reference(oracle, checker, code, edges, nb.METHOD_TEMS, 3, L, shaped, "canonical")], True, (profile, q))
    L = integer_frames(rng, code.N, q)
    gpu_equals(code, nb.METHOD_TEMS, 3, L, plain,
               [reference(oracle, checker, code, edges, nb.METHOD_TEMS, 3, L, plain, m) for m in ("canonical", "literal")], True, (profile, q))


def _odd_code(profile, q):
    """The profile's graph with an odd number of variables, so that odd batches leave idle groups in the last wave of the packed
    variable-node kernel (64 / q variables per wave) at every q <= 32."""
    for M in (12, 13, 14, 15, 16, 17, 18):
        chk, var, once = PROFILES[profile]
        code, edges, _ = degree_code(q, 8100 + q + M, chk, var, M, once=once)
        if code.N % 2:
            return code, edges
    raise AssertionError("no graph with an odd number of variables")


PACKED_CELLS = [(prof, q, m) for prof in ("dv48", "all") for q in (4, 16, 32) for m in ("ems", "tems")
                if not (m == "tems" and (prof, q) in TEMS_REFUSED)]   # (all, GF(32), T-EMS: 40 bits of path code, refused)


@pytest.mark.parametrize("profile,q,method", PACKED_CELLS, ids=[f"{p}-gf{q}-{m}" for p, q, m in PACKED_CELLS])
def test_packed_variable_node_idle_groups_and_mixed_lengths(oracle, checker, profile, q, method):
    """vn_packed_kernel (q <= 32: 64 / q variables per wave): variables of degree 1 .. 8 side by side in one wave (the loop bound
    is the wave's maxdv; shorter variables must add and store nothing past their own edges) and batches whose B * N is not a
    multiple of 64 / q, so that the last wave holds idle groups next to the last codeword.  Batches of 1, 3, 5 and 7 codewords:
    prefix property (a batch decodes like the first rows of the full batch) and the message state of the LAST codeword bit for
    bit against the canonical oracle.  EMS (no damping) and T-EMS (damped: the kernel reads the previous v2c); T-EMS on `all`
    stops at GF(16) (32-bit path code)."""
    code, edges = _odd_code(profile, q)
    meth, _, kw = method_runs(method, q)[0]
    rng = np.random.default_rng(31 * q + len(profile))
    L = rng.normal(-1.5, 3.0, (7, code.N, q - 1))
    L[2] = np.round(L[2])
    ref = reference(oracle, checker, code, edges, meth, 3, L, kw, "canonical")
    assert any((B * code.N) % (64 // q) for B in (1, 3, 5, 7)), "no batch leaves an idle group"
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, meth, 3, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        full = dec.decode(L)
        for B in (1, 3, 5, 7):
            got = dec.decode(L[:B])
            for a, f in zip(got, full):
                assert np.array_equal(a, f[:B]), (variant, B)
            r, o, it, st = ref[B - 1]
            assert (got[1][B - 1], got[2][B - 1]) == (r, it) and np.array_equal(got[0][B - 1], o), (variant, B)
            for k, (a, x) in enumerate(zip(dec.read_state(B - 1), st)):
                if not (k == 1 and r == 1 and it >= 2):
                    assert np.array_equal(a, x), (variant, B, k)
        dec.close()


# Eb/N0 values (dB, in the rate-1/2 convention of _bpsk_llr_zero), chosen on the CPU with the oracle alone so that the
# batch mixes frames that converge at once, late and never on the weak `all` graphs
MIX_EBN0 = (0.0, 2.0, 4.0, 8.0)


def mixed_convergence_batch(q):
    code, edges, _ = profile_code("all", q)
    rng = np.random.default_rng(500 + q)
    L = np.concatenate([_bpsk_llr_zero(rng, code, 6, e) for e in MIX_EBN0], axis=0)
    return code, edges, L


@pytest.mark.parametrize("fixed,poll", [(0, 0), (0, 2), (1, 0)])
@pytest.mark.parametrize("method", ["ems", "bstems"])
@pytest.mark.parametrize("q", [16, 64])
def test_early_exit_fixed_iterations_and_active_list_on_high_degrees(oracle, checker, q, method, fixed, poll):
    """`all` profile (checks 2-8, variables 1-8), 12 iterations: early exit with and without polling, fixed iterations, and the
    active list (batches of 1024 and more with polling re-launch over the codewords still iterating), on all-zero-codeword BPSK
    frames that converge at once, late and never -- the mix is asserted on the ORACLE's flags.  Decisions, flags, iteration
    counts of every frame; message state of every frame of the small batch."""
    code, edges, L = mixed_convergence_batch(q)
    meth, _, kw = method_runs(method, q)[0]
    ref = reference(oracle, checker, code, edges, meth, 12, L, kw, "canonical", fixed=fixed)
    n_conv = sum(r for r, _, _, _ in ref)
    its = sorted({it for r, _, it, _ in ref if r})
    assert 0 < n_conv < L.shape[0], "the batch must mix converged and unconverged codewords"
    assert its[0] == 1 and its[-1] >= 3, ("frames must converge at once and late", its)
    for variant in (0, 1, 2):
        dec = nb.Decoder(code, meth, 12, fixed_iters=fixed, poll_every=poll, **kw)
        _force_generic(dec, variant)
        dec.record_state(True)
        out, conv, n_its = dec.decode(L)
        for b, (r, o, it, st) in enumerate(ref):
            assert (conv[b], n_its[b]) == (r, it) and np.array_equal(out[b], o), (variant, b)
            for k, (a, x) in enumerate(zip(dec.read_state(b), st)):
                if not (k == 1 and r == 1 and it >= 2 and not fixed):
                    assert np.array_equal(a, x), (variant, b, k)
        if poll:  # 1032 codewords: the active list takes over after the first window
            reps = 1032 // L.shape[0]
            big = np.concatenate([L] * reps, axis=0)
            dec.record_state(False)
            out, conv, n_its = dec.decode(big)
            for b in range(big.shape[0]):
                r, o, it, _ = ref[b % L.shape[0]]
                assert (conv[b], n_its[b]) == (r, it) and np.array_equal(out[b], o), (variant, "active list", b)
        dec.close()


RING256 = {"ems": (nb.METHOD_EMS, dict(ems_nm=32, ems_nc=3)), "tems": (nb.METHOD_TEMS, dict(tems_nr=2, tems_nc=3)), "bp": (nb.METHOD_BP, dict())}


@pytest.mark.parametrize("method", ["ems", "tems", "bp"])
@pytest.mark.parametrize("q", [16, 64, 256])
def test_which_iteration_ran(q, method):
    """nbl_last_timing's launch counters: the fused iteration makes no variable-node launch.  dc78 (variables of degree 2 / 3) runs
    fused under the default kernel choice; dv4edge (ONE variable of degree 4) and dv48 take the separate variable-node launch,
    as does every code under variants 1 and 2.  GF(256): an 8-check (2,4) ring, fused under the EMS-256, T-EMS-256 and BP-256
    kernels.  nbl_debug_plan reports the same `fused` for every cell.  (This separates fused from unfused only; WHICH kernel
    serves a shape is pinned by tests/test_plan.py, and that the kernels agree by the three variants against the oracle.)"""
    if q == 256:
        code = ring_code(256, 8, 4)
        cells = [("ring4", True, code) + RING256[method]]
    else:
        cells = []
        for profile, fused in (("dc78", True), ("dv4edge", False), ("dv48", False)):
            if method == "tems" and profile == "dc78" and q == 64:
                continue  # (refused: 6 * 8 bits of path code)
            cells.append((profile, fused, profile_code(profile, q, method)[0]) + method_runs(method, q)[0][:2])
    for tag, fused, code, meth, kw in cells:
        L = np.random.default_rng(q).normal(-1.5, 3.0, (4, code.N, q - 1))
        plan_kw = {k: v for k, v in kw.items() if not k.endswith(("_factor", "_offset"))}
        for variant in (0, 1, 2):
            dec = nb.Decoder(code, meth, 3, fixed_iters=1, **kw)
            _force_generic(dec, variant)
            dec.decode(L)
            _, (n_vn, n_syn, n_cn) = dec.last_timing()
            dec.close()
            assert (n_syn, n_cn) == (3, 3), (tag, variant, n_vn, n_syn, n_cn)
            assert n_vn == (0 if fused and variant == 0 else 3), (tag, variant, n_vn)
            assert debug_plan(code, meth, force_generic=variant, **plan_kw)[2] == (fused and variant == 0), (tag, variant)


@pytest.mark.parametrize("name", DEG_FIXTURES)
def test_fixture_outputs_equal_reference(oracle, checker, name):
    """The deg_* fixtures recorded from the compiled reference on the degree-profile graphs: decisions and flags equal in all three
    kernel variants; message state within 1e-9 of the reference's, and bit-identical to the canonical restatement's for EMS /
    T-EMS / BS-TEMS."""
    g, meta = load_golden(name)
    p = meta["profile"]
    code, edges = spec_edges(meta["spec"])
    meth = p["method"]
    kw = bs_kwargs(p) if meth == nb.METHOD_BS_TEMS else {} if meth == nb.METHOD_BP else \
        {k: v for k, v in decoder_kwargs(p).items() if k.startswith("ems_" if meth == nb.METHOD_EMS else "tems_")}
    L = g["L_ch"]
    for variant in (0, 1, 2):
        for k, it in enumerate(g["iters"]):
            dec = nb.Decoder(code, meth, int(it), **kw)
            _force_generic(dec, variant)
            out, conv, iters = dec.decode(L)
            dec.close()
            assert np.array_equal(out, g["out"][k]), (name, variant, int(it))
            assert np.array_equal(conv, g["syn_ok"][k]), (name, variant, int(it))
            if meth != nb.METHOD_BP:  # (BP's failure return value is undefined in the reference)
                assert np.array_equal(conv, g["ret"][k]), (name, variant, int(it))
        for k, it in enumerate(g["state_iters"]):
            lanes = [int(b) for b in g["state_lanes"]]
            dec = nb.Decoder(code, meth, int(it), **kw)
            _force_generic(dec, variant)
            dec.record_state(True)
            _, conv, iters = dec.decode(L)
            ref = None if meth == nb.METHOD_BP else reference(oracle, checker, code, edges, meth, int(it), L[lanes], kw, "canonical")
            for li, b in enumerate(lanes):
                st = dec.read_state(b)
                v_ok = not (conv[b] and iters[b] >= 2)
                for j, (a, rf) in enumerate(zip(st, (g["st_post"][k, li], g["st_v2c"][k, li], g["st_c2v"][k, li]))):
                    if j != 1 or v_ok:
                        assert np.max(np.abs(a - rf)) <= LLR_TOL * max(1.0, np.max(np.abs(rf))), (name, variant, int(it), b, j)
                        if ref is not None:
                            assert np.array_equal(a, ref[li][3][j]), (name, variant, int(it), b, j)
            dec.close()
