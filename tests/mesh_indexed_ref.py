"""The specification of vh_extract_mesh_indexed in numpy, on the tables and aprons of tests/mesh_ref.py.  It does not
import the product.

Rule (DESIGN.md "mesh", indexed form): the triangles are those of mesh_ref.extract, in its order.  A vertex is its edge
(A, d): A the global voxel of the lower end, d = 1..7 the axes on which the upper end is A + 1.  It exists iff an emitted
triangle uses it.  Vertices are ordered by (entry index of the block that holds A, voxel index of A in it, d); a face holds
the positions of its three edges in that order.  mesh_ref.extract does not return the edge of a triangle corner, so the
part of it that walks the cells is restated here; tests/test_mesh_indexed_cpu.py pins the two together bit for bit."""
import numpy as np

import mesh_ref
from mesh_ref import F, TETS, TRI_E, TRI_N


def _listed(table, region):
    listed = np.nonzero(table["ptr"] != -1)[0]
    if region is not None:
        lo, hi = np.asarray(region[0]), np.asarray(region[1])
        p = table["pos"][listed]
        listed = listed[((p >= lo) & (p < hi)).all(1)]
    return listed


def corners(table, voxels, region=None):
    """Every triangle corner of mesh_ref.extract, in its order: dict of n [T] (position of the cell's block among the
    listed), la, lb [T, 3, 3] local voxel of the two ends in that block (0..8), plus the aprons A and the keys pos."""
    listed = _listed(table, region)
    if len(listed) == 0:
        return None
    A, pos = mesh_ref._aprons(table, voxels, listed)
    cs = np.stack([A[:, 1 + (i >> 2):9 + (i >> 2), 1 + ((i >> 1) & 1):9 + ((i >> 1) & 1), 1 + (i & 1):9 + (i & 1)]
                   for i in range(8)], -1)
    valid = ~np.isnan(cs).any(-1)
    with np.errstate(invalid="ignore"):
        inside = cs <= 0
    cm = (inside.astype(np.int64) << np.arange(8)).sum(-1)
    n, z, y, x = np.nonzero(valid & (cm != 0) & (cm != 255))
    if len(n) == 0:
        return None
    cm = cm[n, z, y, x]
    tm = np.zeros((len(n), 6), np.int64)
    for s in range(4):
        tm |= ((cm[:, None] >> TETS[None, :, s]) & 1) << s
    present = np.arange(2)[None, None, :] < TRI_N[np.arange(6)[None, :], tm][:, :, None]
    e, t, k = np.nonzero(present)
    edges = TRI_E[t, tm[e, t], k]
    ca = TETS[t[:, None], edges[:, :, 0]]
    cb = TETS[t[:, None], edges[:, :, 1]]
    cell = np.stack([x[e], y[e], z[e]], -1)[:, None, :]
    bit = np.arange(3)[None, None, :]
    return {"n": n[e], "la": cell + ((ca[:, :, None] >> bit) & 1), "lb": cell + ((cb[:, :, None] >> bit) & 1),
            "d": ca ^ cb, "A": A, "pos": pos}


def entry_of(table):
    """{block key: entry index} of the allocated entries."""
    at = np.nonzero(table["ptr"] != -1)[0]
    return {tuple(p): int(i) for i, p in zip(at, table["pos"][at].tolist())}


def extract_indexed(table, voxels, voxel_size, region=None, normals=False):
    """(vertices [V, 3] float32, faces [T, 3] int64, normals [V, 3] or None, info).  info: "edge" [V, 5] int64 = (global
    voxel A x, y, z, d, entry index of A's block) per vertex, "corner_edge" the same per triangle corner [T, 3, 5]."""
    tris, nrm, _ = mesh_ref.extract(table, voxels, voxel_size, region, normals=normals)
    c = corners(table, voxels, region)
    none = (np.zeros((0, 3), F), np.zeros((0, 3), np.int64), np.zeros((0, 3), F) if normals else None,
            {"edge": np.zeros((0, 5), np.int64), "corner_edge": np.zeros((0, 3, 5), np.int64)})
    if c is None:
        assert len(tris) == 0
        return none
    assert len(c["n"]) == len(tris)
    ga = c["pos"][c["n"]][:, None, :] * 8 + c["la"]                       # [T, 3, 3] global voxel of A
    where = entry_of(table)
    flat = ga.reshape(-1, 3)
    keys, inv = np.unique(flat >> 3, axis=0, return_inverse=True)
    entry = np.array([where[tuple(k)] for k in keys.tolist()], np.int64)[inv.reshape(-1)]
    voxel = ((flat[:, 2] & 7) << 6) | ((flat[:, 1] & 7) << 3) | (flat[:, 0] & 7)
    d = c["d"].reshape(-1)
    rank = (entry * 512 + voxel) * 8 + d
    order, first, index = np.unique(rank, return_index=True, return_inverse=True)
    verts = np.ascontiguousarray(tris.reshape(-1, 3)[first])
    vn = np.ascontiguousarray(nrm.reshape(-1, 3)[first]) if normals else None
    corner_edge = np.concatenate([flat, d[:, None], entry[:, None]], 1)
    return verts, index.reshape(-1, 3).astype(np.int64), vn, {"edge": corner_edge[first], "corner_edge": corner_edge.reshape(-1, 3, 5)}


def edges_by_rule(table, voxels, region=None):
    """The existence rule from the voxel's side, [V, 5] rows (A x, y, z, d, entry of A's block) in vertex order: the two
    ends are valid with different inside flags, and one of the cells that contain the edge (corner 0 at A - o, o disjoint
    from d) has eight valid corners and lies in a block of the region."""
    alloc = np.nonzero(table["ptr"] != -1)[0]
    A, pos = mesh_ref._aprons(table, voxels, alloc)                       # local -1..9 at index +1
    valid = ~np.isnan(A)
    with np.errstate(invalid="ignore"):
        inside = A <= 0
    N = len(alloc)
    cell_ok = np.ones((N, 9, 9, 9), bool)                                 # cells with corner 0 at local -1..7 (index +1)
    for i in range(8):
        cell_ok &= valid[:, (i >> 2):9 + (i >> 2), ((i >> 1) & 1):9 + ((i >> 1) & 1), (i & 1):9 + (i & 1)]
    if region is not None:
        lo, hi = np.asarray(region[0], np.int64), np.asarray(region[1], np.int64)
        for o in range(8):                                                # the cell's block: key - 1 on the axes where it sits at -1
            off = np.array([o & 1, (o >> 1) & 1, o >> 2])
            k = pos - off
            ok = ((k >= lo) & (k < hi)).all(1)
            sl = tuple(slice(0, 1) if b else slice(1, 9) for b in off[::-1])
            cell_ok[(slice(None),) + sl] &= ok[:, None, None, None]
    rows = []
    for d in range(1, 8):
        dz, dy, dx = d >> 2, (d >> 1) & 1, d & 1
        a = (slice(None), slice(1, 9), slice(1, 9), slice(1, 9))
        b = (slice(None), slice(1 + dz, 9 + dz), slice(1 + dy, 9 + dy), slice(1 + dx, 9 + dx))
        crossing = valid[a] & valid[b] & (inside[a] != inside[b])
        held = np.zeros((N, 8, 8, 8), bool)
        for o in range(8):
            if o & d:
                continue
            oz, oy, ox = o >> 2, (o >> 1) & 1, o & 1
            held |= cell_ok[:, 1 - oz:9 - oz, 1 - oy:9 - oy, 1 - ox:9 - ox]
        n, z, y, x = np.nonzero(crossing & held)
        g = pos[n] * 8 + np.stack([x, y, z], 1)
        rows.append(np.concatenate([g, np.full((len(n), 1), d), alloc[n][:, None]], 1))
    rows = np.concatenate(rows).astype(np.int64)
    voxel = ((rows[:, 2] & 7) << 6) | ((rows[:, 1] & 7) << 3) | (rows[:, 0] & 7)
    return rows[np.argsort((rows[:, 4] * 512 + voxel) * 8 + rows[:, 3], kind="stable")]


def directed_edges(faces):
    """[3T, 2]: the directed edges (i, j) of every triangle."""
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def repeated_directed_edges(faces):
    """How many directed edges occur more than once."""
    e = directed_edges(faces)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return int((counts > 1).sum())


def closed_manifold(faces, num_vertices):
    """(every undirected edge lies in exactly two triangles, V - E + T)."""
    e = np.sort(directed_edges(faces), 1)
    und, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all()), int(num_vertices) - len(und) + len(faces)
