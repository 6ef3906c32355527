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


def _rgb_bytes(colors, count):
    """Per-vertex colours as [V, 3] uint8: from [V, 3] bytes, or from [V] words r | g << 8 | b << 16 (byte 3 dropped)."""
    c = np.asarray(colors)
    if c.ndim == 1:
        c = np.ascontiguousarray(c.astype("<u4")).view(np.uint8).reshape(-1, 4)[:, :3]
    c = np.ascontiguousarray(c, np.uint8).reshape(-1, 3)
    if len(c) != count:
        raise ValueError("colors must be one per vertex")
    return c


def save_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x y z (and nx ny nz with `normals` [V, 3], and uchar red green blue with `colors`,
    [V, 3] bytes or [V] words r | g << 8 | b << 16), faces as uchar-counted int lists."""
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
    payload = np.ascontiguousarray(data, "<f4").tobytes()
    if colors is not None:
        header += [f"property uchar {p}" for p in ("red", "green", "blue")]
        vrec = np.empty(len(vertices), np.dtype([("f", "<f4", (len(props),)), ("c", "u1", (3,))]))
        vrec["f"] = data
        vrec["c"] = _rgb_bytes(colors, len(vertices))
        payload = vrec.tobytes()
    header += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    rec["n"] = 3
    rec["v"] = faces
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(payload)
        f.write(rec.tobytes())


def load_ply(path):
    """The inverse of save_ply (and of SDF_Hashtable::saveMeshPly): (vertices [V, 3], faces [T, 3] int32, normals [V, 3] or None),
    and for a file with `uchar red green blue` a fourth element, the colours [V, 3] uint8."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = nf = 0
    props, element, colored = [], None, []
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
        elif w[0] == "property" and element == "vertex" and w[1] == "uchar":
            colored.append(w[2])
        elif w[0] == "property" and element == "vertex":
            if w[1] != "float" or colored:
                raise ValueError("vertex properties must be float")
            props.append(w[2])
        elif w[0] == "property" and element == "face" and w[1:] != ["list", "uchar", "int", "vertex_indices"]:
            raise ValueError("faces must be `list uchar int vertex_indices`")
    if props[:3] != ["x", "y", "z"] or props[3:] not in ([], ["nx", "ny", "nz"]):
        raise ValueError("unsupported vertex layout")
    k = len(props)
    if colored:
        if colored != ["red", "green", "blue"]:
            raise ValueError("unsupported vertex layout")
        vrec = np.frombuffer(blob, np.dtype([("f", "<f4", (k,)), ("c", "u1", (3,))]), nv, end)
        rec = np.frombuffer(blob, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, end + vrec.nbytes)
        if nf and not (rec["n"] == 3).all():
            raise ValueError("only triangles are supported")
        data = vrec["f"]
        return data[:, :3].copy(), rec["v"].astype(np.int32), (data[:, 3:].copy() if k == 6 else None), vrec["c"].copy()
    data = np.frombuffer(blob, "<f4", nv * k, end).reshape(nv, k)
    rec = np.frombuffer(blob, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, end + 4 * nv * k)
    if nf and not (rec["n"] == 3).all():
        raise ValueError("only triangles are supported")
    return data[:, :3].copy(), rec["v"].astype(np.int32), (data[:, 3:].copy() if k == 6 else None)
