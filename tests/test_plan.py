"""Which check-node kernel serves which shape: nbl_debug_plan (host arithmetic: no device, no decoder) against the table
tests/golden/cn_plan_table.json, recorded from the kernel choice as it stood before the choice moved into nbl_plan.cpp.

A code that drops from a specialised kernel to the general one still passes every parity test (they compare with the oracle);
it only runs several times slower.  This table is what notices.

Grid: every (profile, q) of degree_util, (2, dc)-regular rings (dc 4, 6, 8) at every q, a (3, 4)-regular graph over GF(64),
GF(16) and GF(256) (the GF(256) kernels behind a separate variable-node pass), the ten shipped codes; EMS nm in {8, 32, 64,
65, q} (<= q) x nc in {0, 1, 2, 3, 5}, flooding, layered and layered "damped"; T-EMS (nr, nc) in {(2,2), (2,3), (4,3), (5,3), (2,4)}, flooding and layered damped; log-QSPA; BS-TEMS nm in {4, 16};
method 6.  Per cell four variants: force_generic 0 / 1 / 2, and record_state at force_generic 0.  Cells nbl_create* refuses for
a reason other than the device are left out and counted.  NBL_NO_SMALL=1 (read once per process) is walked over the q <= 64
codes in one child process.

File layout: "cells" names the columns, "patterns" lists the distinct answers of a cell -- four variants, each [kernel, fusable,
fused, want_v2c] -- and "codes" / "codes_no_small" give per code one pattern index per cell, -1 = refused."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np

import nbldpc_amd as nb
from nbldpc_amd.binding import debug_plan
from degree_util import PROFILES, QS, degree_code, profile_code, ring_code

TABLE = os.path.join(ROOT, "tests", "golden", "cn_plan_table.json")
KERNELS = ("ems256", "ems_small", "ems64", "ems", "tems64", "tems256", "tems_small", "tems", "bp256", "bp64", "bp_small", "bp",
           "bstems", "ems_layered", "tems_layered", "none")
VARIANTS = ((0, False), (1, False), (2, False), (0, True))   # (force_generic, record_state)
REFUSED, REFUSED_NO_SMALL = 2177, 2093                       # cells nbl_create* refuses, as recorded with the table


def cells():
    """[(label, method, parameters, layers, damped)]: the columns, the same for every code (EMS nm above q is refused)."""
    out = []
    for nm in (8, 32, 64, 65, "q"):
        for nc in (0, 1, 2, 3, 5):
            for tag, lay in (("", None), ("/layered", False), ("/damped", True)):
                out.append((f"ems nm={nm} nc={nc}{tag}", nb.METHOD_EMS, dict(ems_nm=nm, ems_nc=nc), lay))
    for nr, nc in ((2, 2), (2, 3), (4, 3), (5, 3), (2, 4)):
        for tag, lay in (("", None), ("/damped", True)):
            out.append((f"tems nr={nr} nc={nc}{tag}", nb.METHOD_TEMS, dict(tems_nr=nr, tems_nc=nc), lay))
    out.append(("bp", nb.METHOD_BP, {}, None))
    for nm in (4, 16):
        out.append((f"bstems nm={nm}", nb.METHOD_BS_TEMS, dict(bs_nm=nm, bs_nc=2), None))
    out.append(("osd", nb.METHOD_OSD, dict(osd_order=0), None))
    return out


def codes(max_q=256):
    """[(label, graph for EMS / log-QSPA / BS-TEMS / OSD, graph for T-EMS)]; the two differ where degree_util gives T-EMS
    smaller checks (dv48 over GF(128) and GF(256))."""
    out = []
    for prof in PROFILES:
        for q in QS:
            out.append((f"{prof}/{q}", profile_code(prof, q)[0], profile_code(prof, q, "tems")[0]))
    for dc in (4, 6, 8):
        for q in QS:
            out.append((f"ring{dc}/{q}", ring_code(q, 12, dc)))
    for q in (64, 16, 256):
        out.append((f"reg34/{q}", degree_code(q, 3400 + q, (4,), (3,), 12)[0]))
    for name in sorted(nb.datafiles.codes()):
        out.append((name, nb.Code(name)))
    return [(c[0], c[1], c[-1]) for c in out if c[1].q <= max_q]


_GF = {}


def _accepted(code, method, kw, lay):
    """Does nbl_create* take this cell?  Asked with device -1, which an accepted shape fails on last: 'no device' on a box
    without one, 'device index out of range' on one with -- no decoder is ever made."""
    if code.q not in _GF:
        _GF[code.q] = tuple(np.array(t, dtype=np.uint16) for t in nb.datafiles.gf_tables(code.q))
    extra = {} if lay is None else dict(layers="greedy", damped=lay)
    try:
        nb.Decoder(code, method, 5, device=-1, gf=_GF[code.q], **kw, **extra).close()
    except nb.NblError as e:
        return e.status == -3 or (e.status == -1 and "device index out of range" in str(e))
    raise AssertionError("device -1 made a decoder")


def walk(max_q=256):
    """{code label: [None (refused) | [[kernel, fusable, fused, want_v2c] per variant] per cell]}"""
    table = {}
    for label, code, code_tems in codes(max_q):
        row = []
        for _, method, kw, lay in cells():
            c = code_tems if method == nb.METHOD_TEMS else code
            kw = {k: (c.q if v == "q" else v) for k, v in kw.items()}
            if not _accepted(c, method, kw, lay):
                row.append(None)
                continue
            pk = {k: v for k, v in kw.items() if k != "osd_order"}
            extra = {} if lay is None else dict(layers="greedy", damped=lay)
            row.append([list(debug_plan(c, method, force_generic=fg, record_state=rs, **pk, **extra)) for fg, rs in VARIANTS])
        table[label] = row
    return table


def walk_no_small():
    """walk(64) of a child process that has NBL_NO_SMALL=1 from its start"""
    env = dict(os.environ, NBL_NO_SMALL="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def unpack(stored, key):
    return {label: [None if i < 0 else stored["patterns"][i] for i in row] for label, row in stored[key].items()}


def pack(table, table_no_small):
    patterns = []

    def index(pat):
        if pat is None:
            return -1
        if pat not in patterns:
            patterns.append(pat)
        return patterns.index(pat)
    enc = {key: {label: [index(p) for p in row] for label, row in t.items()} for key, t in (("codes", table), ("codes_no_small", table_no_small))}
    return dict(cells=[c[0] for c in cells()], variants=[list(v) for v in VARIANTS], patterns=patterns, **enc)


def _compare(got, want, tag):
    assert list(got) == list(want), tag
    labels = [c[0] for c in cells()]
    diff = [(tag, code, labels[i], got[code][i], want[code][i]) for code in want for i in range(len(labels)) if got[code][i] != want[code][i]]
    assert not diff, (len(diff), diff[:10])


def test_kernel_choice_equals_the_recorded_table():
    stored = json.load(open(TABLE))
    assert stored["cells"] == [c[0] for c in cells()] and stored["variants"] == [list(v) for v in VARIANTS]
    want, want_ns = unpack(stored, "codes"), unpack(stored, "codes_no_small")
    # the grid reaches every kernel, and under NBL_NO_SMALL exactly the four kernels the switch takes out are gone
    seen = {v[0] for row in want.values() for pat in row if pat for v in pat}
    assert seen == set(KERNELS), sorted(set(KERNELS) ^ seen)
    seen_ns = {v[0] for row in want_ns.values() for pat in row if pat for v in pat}
    assert not seen_ns & {"ems_small", "tems_small", "bp_small", "ems64"} and {"tems64", "bp64", "ems", "tems", "bp"} <= seen_ns
    assert sum(p is None for row in want.values() for p in row) == REFUSED
    assert sum(p is None for row in want_ns.values() for p in row) == REFUSED_NO_SMALL
    _compare(walk(), want, "default")
    _compare(walk_no_small(), want_ns, "NBL_NO_SMALL=1")


def test_plan_invariants():
    """What the issue lists as not to change, read off the recorded table itself (so a re-recorded table cannot move them)."""
    stored = json.load(open(TABLE))
    for key in ("codes", "codes_no_small"):
        for code, row in unpack(stored, key).items():
            for label, pat in zip(stored["cells"], row):
                if pat is None:
                    continue
                (k0, fusable, fused0, v0), (k1, f1, fused1, v1), (k2, f2, fused2, v2), (kr, fr, fusedr, vr) = pat
                tag = (key, code, label)
                assert fusable == f1 == f2 == fr, tag                       # c2v_alt / c2v_zero: the shape decides, no debug switch
                assert fused0 == fusedr == fusable and not fused1 and not fused2, tag
                assert k1 in ("ems", "tems", "bp", "bstems", "ems_layered", "tems_layered", "none"), tag
                assert kr == k0, tag
                if "/" in label or label.startswith(("bstems", "osd")):
                    assert not fusable and k0 == k1 == k2, tag
                if label.startswith("ems") and "/" not in label:
                    assert v0 == (not fused0) and v1 and v2 and vr, tag     # v2c: unfused, read-back, or a debug variant
                elif label.startswith("ems"):
                    assert not (v0 or v1 or v2 or vr), tag                  # layered EMS keeps no v2c
                else:
                    assert v0 and v1 and v2 and vr, tag


def test_plan_unit_under_host_sanitizers(tmp_path):
    """nbl_plan.cpp holds no HIP call: it is compiled here for the host with AddressSanitizer and UBSan into a stand-alone program
    (tests/plan_check.cpp: rows of the table on degree arrays of exactly N and M entries) that takes the nbl_*_applicable predicates
    from the product library, and run."""
    csrc = os.path.join(ROOT, "nbldpc_amd", "csrc")
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tests", "plan_check.cpp"), os.path.join(csrc, "nbl_plan.cpp"), nb.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(nb.LIB_PATH), "-Wl,--allow-shlib-undefined", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), (out.stdout, out.stderr[-2000:])


if __name__ == "__main__":
    json.dump(walk(64), sys.stdout)
