#!/usr/bin/env python3
"""Writes voxelhashing_demo_amd/csrc/vh_mesh_table.h: the marching-tetrahedra table of vh_extract_mesh ("mesh").

Kuhn split of the unit cell: one tetrahedron per permutation (a, b, c) of the axes, corners [0, 1<<a, 1<<a|1<<b, 7]
(corner index = dx | dy<<1 | dz<<2), slots 0..3.  For every set of inside slots the triangles are listed as edges
(lo slot, hi slot) and wound so that the normal points from the inside corners to the outside ones.

One 32-bit word per (tetrahedron, mask): bits 0-1 = number of triangles, then one nibble per vertex
(lo | hi << 2), triangle 0's three vertices first.  Run with --check to compare the committed header with this rule.
"""
import itertools
import os
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "voxelhashing_demo_amd", "csrc", "vh_mesh_table.h")


def tets():
    out = []
    for perm in itertools.permutations(range(3)):
        c, cur = [0], 0
        for a in perm:
            cur |= 1 << a
            c.append(cur)
        out.append(tuple(c))
    return out


def triangles(tet, mask):
    P = [np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1], float) for i in tet]
    ins = [k for k in range(4) if mask >> k & 1]
    out = [k for k in range(4) if not mask >> k & 1]
    tris = []
    if len(ins) == 1:
        tris = [[(ins[0], out[0]), (ins[0], out[1]), (ins[0], out[2])]]
    elif len(ins) == 3:
        tris = [[(ins[0], out[0]), (ins[1], out[0]), (ins[2], out[0])]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    res = []
    for tr in tris:
        pts = [(P[e[0]] + P[e[1]]) / 2 for e in tr]
        n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
        if n @ (np.mean([P[k] for k in out], 0) - np.mean([P[k] for k in ins], 0)) < 0:
            tr = [tr[0], tr[2], tr[1]]
        res.append([(min(e), max(e)) for e in tr])
    return res


def pack(tris):
    w = len(tris)
    for k, tr in enumerate(tris):
        for j, (lo, hi) in enumerate(tr):
            w |= (lo | hi << 2) << (2 + 4 * (3 * k + j))
    return w


def render():
    T = tets()
    lines = ["// vh_mesh_table.h -- marching tetrahedra on the Kuhn split: written by tools/gen_mesh_table.py, do not edit.",
             "// kMeshTet[t]: the cell corners (dx | dy<<1 | dz<<2) of tetrahedron t's slots 0..3, one byte each, slot 0 lowest.",
             "// kMeshTable[t][mask of inside slots]: bits 0-1 = triangles, then a nibble per vertex (lo slot | hi slot << 2).",
             "#pragma once",
             "namespace vh {",
             "__device__ const uint32_t kMeshTet[6] = {" + ", ".join(
                 "0x%08xu" % sum(c << (8 * s) for s, c in enumerate(t)) for t in T) + "};",
             "__device__ const uint32_t kMeshTable[6][16] = {"]
    for t in T:
        lines.append("    {" + ", ".join("0x%08xu" % pack(triangles(t, m)) for m in range(16)) + "},")
    lines += ["};", "}  // namespace vh", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else "vh_mesh_table.h differs from the rule")
    open(HEADER, "w").write(text)
