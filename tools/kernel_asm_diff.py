#!/usr/bin/env python3
"""Build against build: the device assembly of every kernel symbol of two listings of the same unit (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S),
instruction by instruction with operands, local branch labels renumbered in order of appearance.  Prints per kernel 'identical' / 'DIFFERENT' / 'new' / 'gone'
with its instruction count, and for the new kernels the resources the code object records (VGPRs, AGPRs, spills, private segment bytes; LDS is dynamic: K::lds_bytes()).
  python3 tools/kernel_asm_diff.py parent_merkle_tree.s this_merkle_tree.s
--rename 'OLD=NEW' (repeatable) pairs a kernel struct of the first listing with the struct of the second whose name is the first's with OLD replaced by NEW (white
space aside), and reports the pair as 'identical' / 'DIFFERENT' instead of 'gone' and 'new':
  python3 tools/kernel_asm_diff.py a.s b.s --rename 'B2InnerSubtreeKernel=LaneSubtreeKernel<Blake2sNode>' --rename 'KeccakInnerSubtreeKernel<1u>=LaneSubtreeKernel<KeccakNode<1u>>'"""
import argparse
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read().split("\n")
    names = {m.group(1) for l in txt for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    body, res, cur = {}, {}, None
    for l in txt:
        m = re.match(r"^(\S+):", l)
        if m and m.group(1) in names and not l.startswith("\t"):
            cur = m.group(1); body[cur] = []; continue
        if cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
            elif re.match(r"^\t[a-z]", l):
                body[cur].append(re.sub(r"\s*;.*$", "", l.strip()))
            elif re.match(r"^\.LBB\d+_\d+:", l):
                body[cur].append(l.split(":")[0] + ":")
    cur = None
    for l in txt:   # the metadata note: one "  - .agpr_count" entry per kernel
        if l.startswith("  - ."):
            cur = {}
        m = re.match(r"\s+(?:- )?\.(agpr_count|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", l)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
        m = re.match(r"\s+\.name:\s+(\S+)", l)
        if m and cur is not None and m.group(1) in names:
            res[m.group(1)] = cur
    for k, ins in body.items():
        order = {}
        def lab(m):
            return ".L%d" % order.setdefault(m.group(0), len(order))
        body[k] = [re.sub(r"\.LBB\d+_\d+", lab, i) for i in ins]
    return body, res


def demangle(syms):
    out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    short = {}
    for s, d in zip(syms, out):
        m = re.search(r"<(.*)>\(", d)   # void msrt::kernel<K>(K::Params): the kernel struct
        d = m.group(1) if m else d
        short[s] = re.sub(r"\bms(merkle|fri|ctx|field)::", "", d)
    return short


def count(ins):
    return sum(1 for i in ins if not i.endswith(":"))


def renamed(s, names, a, b, renames):
    """the symbol of the second listing that holds the kernel struct `names[s]` of the first under its new name, or None"""
    squeeze = lambda t: re.sub(r"\s+", "", t)
    want = squeeze(names[s])
    for old, new in renames:
        want = want.replace(squeeze(old), squeeze(new))
    if want == squeeze(names[s]):
        return None
    hits = [t for t in b if t not in a and squeeze(names[t]) == want]
    return hits[0] if len(hits) == 1 else None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("first"); ap.add_argument("second")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    a, _ = kernels(args.first)
    b, res = kernels(args.second)
    names = demangle(sorted(set(a) | set(b)))
    print(f"{len(a)} kernels in the first build, {len(b)} in the second")
    bad = 0
    paired = set()
    for s in sorted(a, key=lambda s: names[s]):
        t, label = s, names[s]
        if s not in b and renames:
            t = renamed(s, names, a, b, renames)
            if t is not None:
                paired.add(t); label = f"{names[s].strip()} -> {names[t]}"
        if t is None or t not in b:
            print(f"  gone                              {names[s]}"); bad += 1
        elif a[s] == b[t]:
            print(f"  identical  {count(a[s]):6d} instructions  {label}")
        else:
            print(f"  DIFFERENT  {count(a[s]):6d} -> {count(b[t])} instructions  {label}"); bad += 1
    new = sorted((s for s in b if s not in a and s not in paired), key=lambda s: names[s])
    if new:
        print(f"  added in the second build: {len(new)} kernels")
    for s in new:
        r = res.get(s, {})
        print(f"  new        {count(b[s]):6d} instructions  {r.get('vgpr_count', '?'):>3} VGPRs  {r.get('agpr_count', '?'):>3} AGPRs  {r.get('vgpr_spill_count', '?')} spills  "
              f"{r.get('private_segment_fixed_size', '?')} private bytes  {names[s]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
