#!/usr/bin/env python3
"""Register / LDS footing of every instance of cn_ems_q256_dc4_kernel, and plain instruction counts of one of them, from the
gfx950 assembly of nbl_cn_ems256.hip (the flags of nbldpc_amd/csrc/Makefile).

  python tools/ems256_footing.py [--src FILE] [--parent FILE] [-D NAME=VALUE ...] [--count v_readlane_b32 s_nop v_cmp]

--parent: the same translation unit of another revision (git show REV:nbldpc_amd/csrc/nbl_cn_ems256.hip > FILE, next to the
headers it includes); its figures are printed beside this one's.
"""
import argparse
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nbldpc_amd", "csrc")
FLAGS = ["-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing", "-mllvm", "-enable-pre=false", "--offload-arch=gfx950",
         "-I", CSRC, "-x", "hip", "--cuda-device-only", "-S"]
FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"), ("sgpr_spill", ".sgpr_spill_count"),
          ("vgpr_spill", ".vgpr_spill_count"), ("lds", ".group_segment_fixed_size"))


def assembly(src, defs):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.check_call(["hipcc"] + FLAGS + ["-D" + d for d in defs] + ["-o", out, src], stderr=subprocess.DEVNULL)
        return open(out).read()


def instance(name):
    m = re.search(r"cn_ems_q256_dc4_kernelILi(n?)(\d+)ELb([01])ELi(\d)E", name)
    return ((-1 if m.group(1) else 1) * int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else None


def footing(asm):
    """{(NMT, FUSED, NC): {field: value}} from the code-object metadata"""
    res = {}
    for blk in re.split(r"\n  - (?=\.agpr_count)", asm[asm.index("amdhsa.kernels:"):])[1:]:
        inst = instance(re.search(r"\.name:\s+(\S+)", blk).group(1))
        if inst:
            res[inst] = {k: int(re.search(re.escape(f) + r":\s+(\d+)", blk).group(1)) for k, f in FIELDS}
    return res


def counts(asm, inst, prefixes):
    tag = "cn_ems_q256_dc4_kernelILi%s%dELb%dELi%dE" % ("n" if inst[0] < 0 else "", abs(inst[0]), inst[1], inst[2])
    lines = asm.split("\n")
    a = [i for i, l in enumerate(lines) if l.startswith("_Z") and tag in l.split(":")[0] and ":" in l][0]
    b = [i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end")][0]
    ops = [l.split()[0] for l in lines[a + 1:b] if l.startswith("\t") and not l.strip().startswith((";", "."))]
    return {p: sum(o.startswith(p) for o in ops) for p in prefixes}, len(ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(CSRC, "nbl_cn_ems256.hip"))
    ap.add_argument("--parent")
    ap.add_argument("-D", dest="defs", action="append", default=[])
    ap.add_argument("--count", nargs="*", default=["v_readlane_b32", "s_nop", "v_cmp"])
    ap.add_argument("--headline", default="32,1,3")
    a = ap.parse_args()
    head = tuple(int(x) for x in a.headline.split(","))
    asm = assembly(a.src, a.defs)
    new = footing(asm)
    pasm = assembly(a.parent, []) if a.parent else None
    old = footing(pasm) if pasm else {}
    fmt = lambda d: " ".join(f"{k} {d[k]:3d}" for k, _ in FIELDS)
    print("cn_ems_q256_dc4_kernel<NMT, FUSED, NC>: code-object metadata of hipcc --offload-arch=gfx950 -S (the flags of nbldpc_amd/csrc/Makefile)"
          + (", defines " + " ".join(a.defs) if a.defs else "") + (", this change | parent" if old else ""))
    print("(NMT < 0: run-time nm on the layout of -NMT)")
    for inst in sorted(new):
        print(f"{str(inst):13s} {fmt(new[inst])}" + (f"  |  parent {fmt(old[inst])}" if inst in old else ""))
    c, n = counts(asm, head, a.count)
    print(f"static instruction counts of {head}: " + ", ".join(f"{k} {v}" for k, v in c.items()) + f", all {n}"
          + ("" if not pasm else "  |  parent " + ", ".join(f"{k} {v}" for k, v in counts(pasm, head, a.count)[0].items()) + f", all {counts(pasm, head, a.count)[1]}"))


if __name__ == "__main__":
    main()
