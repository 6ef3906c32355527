"""The specification of vh_extract_mesh in vectorised numpy (float32 throughout): marching tetrahedra on the Kuhn split of
every cell whose eight corner voxels are valid, over the arrays any table gives (hash_table(), sdf_blocks(), voxelSize).
It does not import the product.  Output order: blocks in ascending entry index, cells in ascending voxel index inside the
block, tetrahedra 0..5, triangles in table order.

Rule (DESIGN.md "mesh"): voxel (x,y,z) lives in block (x>>3, y>>3, z>>3) at index ((z&7)<<6)|((y&7)<<3)|(x&7); valid iff
its block is in the table and weight > 0; inside iff sdf <= 0.  Cell corners i = dx | dy<<1 | dz<<2.  One tetrahedron per
permutation (a,b,c) of the axes in itertools order, corners [0, 1<<a, 1<<a|1<<b, 7] = slots 0..3.  A vertex lies on the
edge between corners A (subset) and B: t = sA / (sA - sB), coordinate A_k + t where B_k = A_k + 1, times voxelSize."""
import itertools

import numpy as np

F = np.float32


def kuhn_tets():
    tets = []
    for perm in itertools.permutations(range(3)):
        c, cur = [0], 0
        for a in perm:
            cur |= 1 << a
            c.append(cur)
        tets.append(tuple(c))
    return tets


def corner_xyz(i):
    return np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])


def tet_triangles(tet, mask):
    """Triangles of one tetrahedron for the set `mask` of inside slots: lists of three (slot, slot) edges, wound so that
    the normal points from the inside corners to the outside ones."""
    P = [corner_xyz(i).astype(float) for i in tet]
    ins = [k for k in range(4) if mask >> k & 1]
    out = [k for k in range(4) if not mask >> k & 1]
    tris = []
    if len(ins) == 1:
        a = ins[0]
        tris = [[(a, out[0]), (a, out[1]), (a, out[2])]]
    elif len(ins) == 3:
        d = out[0]
        tris = [[(ins[0], d), (ins[1], d), (ins[2], d)]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    fixed = []
    for tr in tris:
        pts = [(P[e[0]] + P[e[1]]) / 2 for e in tr]
        n = np.cross(pts[1] - pts[0], pts[2] - pts[0])
        towards = np.mean([P[k] for k in out], 0) - np.mean([P[k] for k in ins], 0)
        if n @ towards < 0:
            tr = [tr[0], tr[2], tr[1]]
        fixed.append([(min(e), max(e)) for e in tr])
    return fixed


def build_table():
    """{(tetrahedron, mask): triangles}, edges as (lower slot, higher slot)."""
    return {(ti, m): tet_triangles(t, m) for ti, t in enumerate(kuhn_tets()) for m in range(16)}


def packed_table():
    """The table as the library stores it: one word per (tetrahedron, mask), bits 0-1 = triangles, then a nibble per vertex
    (lower slot | higher slot << 2), and the corner bytes of the tetrahedra."""
    tab = build_table()
    words = np.zeros((6, 16), np.uint32)
    for (t, m), tris in tab.items():
        w = len(tris)
        for k, tr in enumerate(tris):
            for j, (lo, hi) in enumerate(tr):
                w |= (lo | hi << 2) << (2 + 4 * (3 * k + j))
        words[t, m] = w
    tets = np.array([sum(c << (8 * s) for s, c in enumerate(t)) for t in kuhn_tets()], np.uint32)
    return tets, words


TETS = np.array(kuhn_tets(), np.int64)                       # [6, 4] corner of slot
_TAB = build_table()
TRI_N = np.array([[len(_TAB[(t, m)]) for m in range(16)] for t in range(6)], np.int64)
TRI_E = np.zeros((6, 16, 2, 3, 2), np.int64)                 # [tet, mask, triangle, vertex, (lo slot, hi slot)]
for (_t, _m), _tris in _TAB.items():
    for _k, _tr in enumerate(_tris):
        TRI_E[_t, _m, _k] = _tr


def _aprons(table, voxels, listed):
    """[N, 11, 11, 11] (z, y, x; local coordinates -1..9 at index +1): sdf of the valid voxels around each listed block,
    NaN where a voxel is not valid."""
    alloc = np.nonzero(table["ptr"] != -1)[0]
    M = len(alloc)
    ptr = table["ptr"][alloc].astype(np.int64)
    vox = voxels[ptr[:, None] + np.arange(512)[None, :]]
    V = np.full((M + 1, 8, 8, 8), np.nan, F)
    V[:M] = np.where(vox["weight"] > 0, vox["sdf"], F(np.nan)).reshape(M, 8, 8, 8)
    where = {tuple(p): i for i, p in enumerate(table["pos"][alloc].tolist())}
    pos = table["pos"][listed].astype(np.int64)
    A = np.full((len(listed), 11, 11, 11), np.nan, F)
    dst = {-1: slice(0, 1), 0: slice(1, 9), 1: slice(9, 11)}
    src = {-1: slice(7, 8), 0: slice(0, 8), 1: slice(0, 2)}
    for oz, oy, ox in itertools.product((-1, 0, 1), repeat=3):
        nb = np.array([where.get((p[0] + ox, p[1] + oy, p[2] + oz), M) for p in pos.tolist()], np.int64)
        A[:, dst[oz], dst[oy], dst[ox]] = V[nb][:, src[oz], src[oy], src[ox]]
    return A, pos


def _gradient(A, n, lx, ly, lz, here):
    """The rule of dda_normal at local voxel (lx, ly, lz) of block n: [K, 3] float32 and ok [K]."""
    g = np.zeros((len(n), 3), F)
    ok = np.ones(len(n), bool)
    for a in range(3):
        d = [int(a == 0), int(a == 1), int(a == 2)]
        sp = A[n, lz + 1 + d[2], ly + 1 + d[1], lx + 1 + d[0]]
        sm = A[n, lz + 1 - d[2], ly + 1 - d[1], lx + 1 - d[0]]
        hp, hm = ~np.isnan(sp), ~np.isnan(sm)
        with np.errstate(invalid="ignore"):
            central = (sp - sm) * F(0.5)
            fwd = sp - here
            bwd = here - sm
        g[:, a] = np.where(hp & hm, central, np.where(hp, fwd, np.where(hm, bwd, F(0))))
        ok &= hp | hm
    return g, ok


def extract(table, voxels, voxel_size, region=None, normals=False):
    """table: VoxelEntry array (pos, ptr, ...) of one context; voxels: its Voxel array (sdf, weight) addressed by ptr.
    region: ((lo3), (hi3)) in blocks, lo <= key < hi, or None.
    Returns (triangles [T, 3, 3] float32, normals [T, 3, 3] float32 or None, info) with info["cells"] = cells with a sign
    change that emit, info["blocks"] = listed blocks, info["block"] = [T, 3] the block key of each triangle, info["cell"] = [T, 3] its cell (voxel of corner 0)."""
    vs = F(voxel_size)
    listed = np.nonzero(table["ptr"] != -1)[0]
    if region is not None:
        lo, hi = np.asarray(region[0]), np.asarray(region[1])
        p = table["pos"][listed]
        listed = listed[((p >= lo) & (p < hi)).all(1)]
    empty = (np.zeros((0, 3, 3), F), np.zeros((0, 3, 3), F) if normals else None,
             {"cells": 0, "blocks": len(listed), "block": np.zeros((0, 3), np.int64), "cell": np.zeros((0, 3), np.int64)})
    if len(listed) == 0:
        return empty
    A, pos = _aprons(table, voxels, listed)
    corners = np.stack([A[:, 1 + (i >> 2):9 + (i >> 2), 1 + ((i >> 1) & 1):9 + ((i >> 1) & 1), 1 + (i & 1):9 + (i & 1)]
                        for i in range(8)], -1)                                    # [N, 8, 8, 8, corner]
    valid = ~np.isnan(corners).any(-1)
    with np.errstate(invalid="ignore"):
        inside = corners <= 0
    cm = (inside.astype(np.int64) << np.arange(8)).sum(-1)
    n, z, y, x = np.nonzero(valid & (cm != 0) & (cm != 255))                       # block order, then voxel index order
    if len(n) == 0:
        return empty
    cm = cm[n, z, y, x]
    tm = np.zeros((len(n), 6), np.int64)
    for s in range(4):
        tm |= ((cm[:, None] >> TETS[None, :, s]) & 1) << s
    t_idx = np.arange(6)[None, :]
    present = np.arange(2)[None, None, :] < TRI_N[t_idx, tm][:, :, None]           # [E, 6, 2]
    e, t, k = np.nonzero(present)                                                  # cell, tetrahedron, triangle: output order
    edges = TRI_E[t, tm[e, t], k]                                                  # [T, 3, 2] slots
    ca = TETS[t[:, None], edges[:, :, 0]]                                          # [T, 3] cell corner of the lower slot
    cb = TETS[t[:, None], edges[:, :, 1]]
    nn = np.broadcast_to(n[e][:, None], ca.shape)
    cell = np.stack([x[e], y[e], z[e]], -1)[:, None, :]                            # [T, 1, 3]
    bit = np.arange(3)[None, None, :]
    la = cell + ((ca[:, :, None] >> bit) & 1)                                      # [T, 3, 3] local voxel of A
    lb = cell + ((cb[:, :, None] >> bit) & 1)
    sA = A[nn, la[..., 2] + 1, la[..., 1] + 1, la[..., 0] + 1]
    sB = A[nn, lb[..., 2] + 1, lb[..., 1] + 1, lb[..., 0] + 1]
    tt = (sA / (sA - sB)).astype(F)
    ga = (pos[n[e]][:, None, :] * 8 + la).astype(F)                                # global voxel of A, exact in float32
    moved = (ga + tt[..., None]).astype(F)
    tris = (np.where(lb != la, moved, ga) * vs).astype(F)
    info = {"cells": len(n), "blocks": len(listed), "block": pos[n[e]], "cell": pos[n[e]] * 8 + cell[:, 0, :]}
    if not normals:
        return tris, None, info
    flat = lambda a: a.reshape(-1)
    gA, okA = _gradient(A, flat(nn), flat(la[..., 0]), flat(la[..., 1]), flat(la[..., 2]), flat(sA))
    gB, okB = _gradient(A, flat(nn), flat(lb[..., 0]), flat(lb[..., 1]), flat(lb[..., 2]), flat(sB))
    tf = flat(tt)[:, None]
    nv = (gA + (tf * (gB - gA)).astype(F)).astype(F)
    length = np.sqrt(((nv[:, 0] * nv[:, 0]).astype(F) + (nv[:, 1] * nv[:, 1]).astype(F)).astype(F)
                     + (nv[:, 2] * nv[:, 2]).astype(F)).astype(F)
    good = okA & okB & (length > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = (nv / length[:, None]).astype(F)
    nrm = np.where(good[:, None], unit, F(0)).astype(F).reshape(tris.shape)
    return tris, nrm, info


def weld(tris):
    """Exact welding: (vertices [V, 3], faces [T, 3])."""
    flat = np.ascontiguousarray(tris.reshape(-1, 3))
    verts, inv = np.unique(flat.view(np.uint32), axis=0, return_inverse=True)
    return verts.view(F), inv.reshape(-1, 3).astype(np.int64)
