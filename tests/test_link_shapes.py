"""The table of tests/link_shapes.py and the host link chain (nbldpc_amd/host) on it, against what the COMPILED REFERENCE's own chain
produced on the same graphs (tests/golden/link_shape_*.npz): transmitted codewords, messages, sigma and channel LLRs bit for bit.
This is what lets tests/test_gpu_link_shapes.py take the host chain as the reference for what the fixtures do not hold."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD, load_golden
import link_shapes as ls
from link_util import prepare_spec_workdir
from nbldpc_amd import hostlib

WITH_FIXTURE = [n for n in ls.SHAPES if n not in ls.NO_REFERENCE]


def test_every_shape_has_a_fixture():
    for name in WITH_FIXTURE:
        assert os.path.exists(os.path.join(GOLD, f"link_shape_{name}.npz")), name
    for tag in ls.stride_cases():
        assert os.path.exists(os.path.join(GOLD, f"link_shape_stride_{tag}.npz")), tag
    # the only shapes without one are those the compiled reference cannot initialise: crcLen 0
    assert all(ls.SHAPES[n]["crc_len"] == 0 for n in ls.NO_REFERENCE)
    assert all(ls.SHAPES[n]["crc_len"] in (8, 16, 24) for n in WITH_FIXTURE)
    assert set(ls.FER_SHAPES) <= set(WITH_FIXTURE)


@pytest.mark.parametrize("name", sorted(ls.SHAPES))
def test_shape_has_the_property_it_is_in_the_table_for(name):
    code, spec, info = ls.shape(name)   # (asserts)
    g = [n for n, r in enumerate(spec["var_rows"]) if len(r) == ls.SHAPES[name].get("punct", 0)]
    assert g == info["punct"]


def test_table_covers_what_the_shipped_codes_do_not():
    infos = {n: ls.shape(n)[2] for n in ls.SHAPES}
    assert {2, 3, 5, 7} <= {i["p"] for i in infos.values()}
    assert any(i["Np"] < 64 for i in infos.values()) and any(i["Np"] % 256 for i in infos.values() if i["Np"] > 256)
    assert any(0 < i["nb"] < 64 for i in infos.values()) and {1, 63} <= {i["nb"] % 64 for i in infos.values() if i["nb"] > 64}
    assert {1, 65} <= {i["K"] for i in infos.values()} and any(i["nb"] == 0 for i in infos.values())
    assert any(i["L"] % 2 and i["order"] == 2 for i in infos.values()) and any(i["L"] < 64 for i in infos.values())
    assert {4, 8, 16, 32, 128} <= {i["q"] for i in infos.values() if i["order"] == i["q"]}
    assert any(i["punct"] and i["order"] == i["q"] for i in infos.values())
    assert any(left < i["K"] for i in infos.values() for _, left in i["swaps"])


@pytest.mark.parametrize("name", ls.FIELD_SHAPES)
def test_field_shapes_send_what_the_default_table_would_not(tmp_path, name):
    """The two shapes with another modulus: their fixture (the compiled reference run on tables of that modulus) differs from what
    the host chain sends with the default tables on the same graph, so a chain that ignored the table files would fail
    test_host_chain_bit_exact; and the generator matrix is H's null space under the shape's table, not under the default one."""
    import nbldpc_amd.datafiles as df
    g, meta = load_golden(f"link_shape_{name}")
    poly = ls.poly_of(name)
    q = ls.SHAPES[name]["q"]
    assert poly == meta["poly"] and df.is_primitive(q, poly) and poly != df.PRIMITIVE_POLY[q]
    _, spec, info = ls.shape(name)
    prepare_spec_workdir(str(tmp_path / "d"), meta["profile"], spec, np.array(meta["points"]))
    _, tx, _, _ = hostlib.frontend(str(tmp_path / "d"), meta["ebn0"], meta["frames"], spec["N"], info["K"], q, meta["profile"]["parallel"])
    assert not np.array_equal(tx, g["tx_code"])
    prepare_spec_workdir(str(tmp_path / "a"), meta["profile"], spec, np.array(meta["points"]), poly=poly)
    gen = hostlib.generator(str(tmp_path / "a"), spec["N"], info["K"])
    syn = {}
    for tag, (mul, _) in (("own", ls.gf_np(q, poly)), ("default", ls.gf_np(q))):
        s = np.zeros((spec["M"], info["K"]), dtype=np.int64)
        for m, row in enumerate(spec["chk_rows"]):
            for v, h in row:
                s[m] ^= mul[h, gen[v - 1].astype(np.int64)]       # gen [N][K]: code[n] = sum_k gen[n][k] msg[k]
        syn[tag] = s
    assert not syn["own"].any() and syn["default"].any()


def test_stride_cases_follow_the_period_of_the_host_register():
    T = ls.pn_period()
    s0 = hostlib.pn_initial(0)
    assert hostlib.pn_clock(s0, T) == s0 and all(hostlib.pn_clock(s0, k) != s0 for k in range(1, T))
    assert sorted(ls.stride_cases().values()) == [T - 1, T, T + 1, 2 * T]


def _host(tmp_path, meta):
    spec, p = meta["spec"], meta["profile"]
    prepare_spec_workdir(str(tmp_path), p, spec, np.array(meta["points"]), poly=meta.get("poly"))
    return hostlib.frontend(str(tmp_path), meta["ebn0"], meta["frames"], spec["N"], spec["N"] - spec["M"], spec["q"], p["parallel"])


@pytest.mark.parametrize("name", WITH_FIXTURE)
def test_host_chain_bit_exact(tmp_path, name):
    g, meta = load_golden(f"link_shape_{name}")
    assert meta["spec"] == json.loads(json.dumps(ls.shape(name)[1])) and meta["profile"] == ls.profile_of(name, meta["profile"]["parallel"])
    assert np.array_equal(np.array(meta["points"]), ls.points_of(name)) and meta.get("poly") == ls.poly_of(name)
    L, tx, msg, sigma = _host(tmp_path, meta)
    assert sigma == g["sigma"][0]
    assert np.array_equal(tx, g["tx_code"])
    assert np.array_equal(msg, g["tx_msg"])
    assert np.array_equal(L.view(np.uint64), g["L_ch"].view(np.uint64))   # bit-identical doubles


@pytest.mark.parametrize("tag", sorted(ls.stride_cases()))
def test_host_chain_bit_exact_at_lane_strides_around_the_period(tmp_path, tag):
    g, meta = load_golden(f"link_shape_stride_{tag}")
    P = meta["profile"]["parallel"]
    assert P == ls.stride_cases()[tag] and meta["spec"] == json.loads(json.dumps(ls.shape(ls.SMALLEST)[1]))
    L, tx, msg, sigma = _host(tmp_path, meta)
    assert sigma == g["sigma"][0]
    assert np.array_equal(tx, g["tx_code"]) and np.array_equal(msg, g["tx_msg"])
    n = meta["lch_lanes"]
    assert np.array_equal(L[:n].view(np.uint64), g["L_ch"].view(np.uint64))
    constant = P % ls.pn_period() == 0
    assert constant == (tag in ("period", "twice_period")) and (constant or len(np.unique(tx, axis=0)) > 2)
    if constant:
        # why the case exists: a stride of whole periods draws the same register output for every message bit of a lane
        _, _, info = ls.shape(ls.SMALLEST)
        for lane in (0, 1, P // 2, P - 1):
            s, bits = hostlib.pn_initial(lane), []
            for _ in range(info["nb"]):
                s = hostlib.pn_clock(s, P - 1)
                bits.append((s >> 9) & 1)          # GenPN puts out regPN[10] after its shift: bit 9 in front of it
                s = hostlib.pn_clock(s, 1)
            assert len(set(bits)) == 1, (lane, bits)
        # so the chain sends two codewords only (the all-zero and the all-one draw), and both occur
        assert len(np.unique(tx, axis=0)) == 2 and not tx[np.argmin(tx.sum(axis=1))].any()
