"""The CPU checker tests/osd_check.cpp against the compiled reference's OSD fixtures (tests/golden/osd_*.npz), and the GF element
matrices of nbldpc_amd.datafiles against the multiplication table.  No GPU."""
import glob
import os

import numpy as np
import pytest

import nbldpc_amd as nb
from conftest import GOLD, load_golden
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


@pytest.mark.parametrize("name", SETS)
def test_checker_equals_reference_on_every_osd_frame(checker, name):
    g, meta = load_golden(name)
    p = profile(meta)
    code = nb.Code(meta["code"])
    kw = osd_kwargs(p)
    L = g["L_ch"]
    checked = 0
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
