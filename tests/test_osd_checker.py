"""The CPU checker tests/osd_check.cpp against the compiled reference's OSD fixtures (tests/golden/osd_*.npz), and the GF element
matrices of nbldpc_amd.datafiles against the multiplication table.  No GPU."""
import glob
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from conftest import GOLD, load_golden
from degree_util import spec_edges
from osd_util import build_checker, decide, flag0_sums, osd_kwargs, profile, run_checker

SETS = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "osd_*.npz")))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("osd"))


@pytest.mark.parametrize("q", [4, 16, 64, 256])
def test_gf_matrices_are_the_binary_image_of_multiplication(q):
    mul, _ = nb.datafiles.gf_tables(q)
    p = q.bit_length() - 1
    full = nb.datafiles.gf_matrices(q, as_loaded=False)
    loaded = nb.datafiles.gf_matrices(q)
    assert full.shape == (q, p, p) and not full[0].any()
    for e in range(1, q):
        for x in range(q):
            bits = [(x >> l) & 1 for l in range(p)]
            y = sum((int(np.dot(bits, full[e][:, k])) & 1) << k for k in range(p))  # column k of row l: bit k of e * 2^l
            assert y == mul[e][x], (q, e, x)
    # CGF::Initial reads q-2 of the q-1 matrices (GF.cpp:137): the element alpha^(q-2) keeps a zero matrix
    last = 1
    for _ in range(q - 2):
        last = mul[last][2]
    assert not loaded[last].any() and full[last].any()
    others = [e for e in range(q) if e != last]
    assert np.array_equal(loaded[others], full[others])


def test_fixtures_cover_the_issue_grid():
    assert len(SETS) >= 7
    seen = {(profile(load_golden(s)[1])["method"]) for s in SETS}
    assert seen == {1, 2, 4, 6, 7}


def test_shape_fixtures_cover_the_issue_grid():
    """osd_shape_*: the shapes, orders and the flag-0 set the fixtures must hold."""
    import osd_shapes as sh
    metas = {s: load_golden(s) for s in SETS if s.startswith("osd_shape_")}
    shapes = {m["shape"] for _, m in metas.values()}
    assert shapes >= {"gf8_odd", "gf8_trunc", "trunc_on_boundary", "gf128", "just_over_64", "just_over_512", "below_cap", "cap", "k1", "k2",
                      "high_rate", "low_rate", "one_word", "irregular"} | set(sh.CRC_PARTIAL)
    flag0 = [m["shape"] for _, m in metas.values() if m["profile"]["osd_flag"] == 0]
    assert any(sh.SHAPES[x]["q"] == 8 for x in flag0)
    for name, (g, m) in metas.items():
        if m["profile"]["osd_flag"] == 1:
            want = {0, 1, 2} | ({3, 5} if sh.shape(m["shape"])[3]["k"] <= 64 else set())
            assert set(g["orders"].tolist()) == want, name
        assert np.array_equal(g["L_ch"], sh.fixture_frames(m["shape"])), name   # (the frames the GPU tests' coverage was chosen on)


@pytest.mark.parametrize("name", SETS)
def test_checker_equals_reference_on_every_osd_frame(checker, name):
    g, meta = load_golden(name)
    p = profile(meta)
    kw = osd_kwargs(p)
    L = g["L_ch"]
    checked = 0
    if "spec" in meta:
        # a synthetic shape (tests/osd_shapes.py): several orders in one file, method 6 on every frame and EMS post-processing
        code, _ = spec_edges(meta["spec"])
        for o in g["orders"]:
            o = int(o)
            B = g[f"out_o{o}"].shape[1]   # (order 2 at n >= 897: the first frames only, the reference's time)
            if p["osd_flag"] == 1:
                c_out = run_checker(checker, code, L[:B], o, 1, kw["crc_len"], kw["crc_rows"])
                assert np.array_equal(c_out, g[f"out_m6_o{o}"]), (name, o, "method 6")
                checked += B
            for k, T in enumerate(g["iters"]):
                lanes = np.flatnonzero(g[f"ret_o{o}"][k] == 0)
                if p["osd_flag"] == 1:
                    assert np.array_equal(c_out[lanes], g[f"out_o{o}"][k][lanes]), (name, o, int(T))
                else:
                    st = list(g["state_iters"])
                    posts = [[g["st_post"][st.index(t), b] for t in range(1, int(T) + 1)] for b in lanes]
                    S = np.array([flag0_sums(ps, p["osd_factor"]) for ps in posts])
                    base = np.array([decide(ps[-1]) for ps in posts])
                    f_out = run_checker(checker, code, L[lanes], o, 0, kw["crc_len"], kw["crc_rows"], S=S, base=base)
                    assert np.array_equal(f_out, g[f"out_o{o}"][k][lanes]), (name, o, int(T))
                checked += len(lanes)
        assert checked > 0, name
        return
    code = nb.Code(meta["code"])
    if p["osd_flag"] == 1 or p["method"] == 6:
        c_out = run_checker(checker, code, L, kw["osd_order"], 1, kw["crc_len"], kw["crc_rows"])
        for k in range(len(g["iters"])):
            lanes = np.arange(L.shape[0]) if p["method"] == 6 else np.flatnonzero(g["ret"][k] == 0)
            assert np.array_equal(c_out[lanes], g["out"][k][lanes]), (name, int(g["iters"][k]))
            checked += len(lanes)
    else:
        # flag 0: S and the base word of frame 0 rebuilt from the reference's own posteriors after 1 .. T iterations
        st = list(g["state_iters"])
        for k, T in enumerate(g["iters"]):
            T = int(T)
            if g["ret"][k][0] or T not in st:
                continue
            posts = [g["st_post"][st.index(t), 0] for t in range(1, T + 1)]
            S = flag0_sums(posts, p["osd_factor"])
            base = decide(posts[-1])
            c_out = run_checker(checker, code, L[:1], kw["osd_order"], 0, kw["crc_len"], kw["crc_rows"], S=S[None], base=base[None])
            assert np.array_equal(c_out[0], g["out"][k][0]), (name, T)
            checked += 1
    assert checked > 0, name
