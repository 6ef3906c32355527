"""Meshes on the host: exact welding of a triangle list and binary little-endian PLY files.  numpy only."""
from __future__ import annotations

import numpy as np


def weld_triangles(tris):
    """[T, 3, 3] float32 -> (vertices [V, 3] float32, faces [T, 3] int32, first [V]): rows with equal bits are one vertex
    (vh_extract_mesh computes a vertex from its edge alone, so shared vertices are bit-equal); first[v] = index of one
    occurrence of vertex v in tris.reshape(-1, 3)."""
    flat = np.ascontiguousarray(np.asarray(tris, np.float32).reshape(-1, 3))
    if len(flat) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0,), np.int64)
    verts, first, inverse = np.unique(flat.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    return verts.view(np.float32), inverse.reshape(-1, 3).astype(np.int32), first


def save_ply(path, vertices, faces, normals=None):
    """Binary little-endian PLY: float x y z (and nx ny nz with `normals` [V, 3]), faces as uchar-counted int lists."""
    vertices = np.asarray(vertices, "<f4").reshape(-1, 3)
    faces = np.asarray(faces, "<i4").reshape(-1, 3)
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError("face index out of range")
    props = ["x", "y", "z"]
    data = vertices
    if normals is not None:
        normals = np.asarray(normals, "<f4").reshape(-1, 3)
        if normals.shape != vertices.shape:
            raise ValueError("normals must be one per vertex")
        props += ["nx", "ny", "nz"]
        data = np.concatenate([vertices, normals], 1)
    header = ["ply", "format binary_little_endian 1.0", "comment voxelhashing_demo_amd", f"element vertex {len(vertices)}"]
    header += [f"property float {p}" for p in props]
    header += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rec["n"] = 3
    rec["v"] = faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(data, "<f4").tobytes())
        f.write(rec.tobytes())


def load_ply(path):
    """The inverse of save_ply (and of SDF_Hashtable::saveMeshPly): (vertices [V, 3], faces [T, 3] int32, normals [V, 3] or None)."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = nf = 0
    props, element = [], None
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            elif element == "face":
                nf = int(w[2])
        elif w[0] == "property" and element == "vertex":
            if w[1] != "float":
                raise ValueError("vertex properties must be float")
            props.append(w[2])
        elif w[0] == "property" and element == "face" and w[1:] != ["list", "uchar", "int", "vertex_indices"]:
            raise ValueError("faces must be `list uchar int vertex_indices`")
    if props[:3] != ["x", "y", "z"] or props[3:] not in ([], ["nx", "ny", "nz"]):
        raise ValueError("unsupported vertex layout")
    k = len(props)
    data = np.frombuffer(blob, "<f4", nv * k, end).reshape(nv, k)
    rec = np.frombuffer(blob, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, end + 4 * nv * k)
    if nf and not (rec["n"] == 3).all():
        raise ValueError("only triangles are supported")
    return data[:, :3].copy(), rec["v"].astype(np.int32), (data[:, 3:].copy() if k == 6 else None)
