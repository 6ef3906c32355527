#!/usr/bin/env python3
"""Register / spill / occupancy summary of the kernels whose name contains one of the given substrings
(from voxelhashing_demo_amd/build/resource_usage.txt, written by `make -C voxelhashing_demo_amd/csrc asm`).

    resources.py [SUBSTRING ...]
    resources.py --compare BEFORE_DIR AFTER_DIR [ALLOWED_SUBSTRING ...]

--compare takes two build directories (resource_usage.txt and vh_kernels.s in each) and prints every kernel whose
resource line and every function whose instruction text (comments, labels and directives dropped) differs, or that
exists on one side only; it exits 1 if one of them contains none of the allowed substrings."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resources(build):
    """kernel name -> its resource line"""
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(os.path.join(build, "resource_usage.txt")).read())[1:]:
        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else None
        scratch, occ, lds = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")
        out[b.split()[0]] = (f"sgpr {g('SGPRs')} vgpr {g('VGPRs')} sspill {g('SGPRs Spill')} vspill {g('VGPRs Spill')} "
                             f"scratch {scratch} occ {occ} lds {lds}")
    return out


def functions(build):
    """function name -> its instructions; a branch target keeps its number inside the function only"""
    out, name = {}, None
    for line in open(os.path.join(build, "vh_kernels.s")):
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line and not line.endswith(":") and not line.startswith("."):
            out[name].append(line)
    return out


def compare(before, after, allowed):
    bad = 0
    for what, a, b in (("resources", resources(before), resources(after)), ("text", functions(before), functions(after))):
        names = sorted(set(a) | set(b))
        moved = [n for n in names if a.get(n) != b.get(n)]
        print(f"{what}: {len(names)} functions, {len(moved)} differ")
        for n in moved:
            ok = any(w in n for w in allowed)
            bad += not ok
            print(f"  {'allowed' if ok else 'MOVED  '} {n[:120]}")
            if what == "resources":
                print(f"          before: {a.get(n)}\n          after:  {b.get(n)}")
    return 1 if bad else 0


if sys.argv[1:2] == ["--compare"]:
    sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4:]))
want = sys.argv[1:] or [""]
for name, line in resources(os.path.join(ROOT, "voxelhashing_demo_amd", "build")).items():
    if any(w in name for w in want):
        print(f"{name[:90]:90s} {line}")
