"""A live mesh of the fused model, kept block by block on the host, in the spirit of streaming.BlockStore: the
policy on top of two exact calls.  vh_changes says which blocks differ from what the cache last saw, were removed, or read a
changed neighbour; vh_extract_mesh_blocks gives the triangles of exactly those.  After update() the chunk of every allocated
block holds the bytes a full extraction would give it, whatever calls changed the model in between."""
from __future__ import annotations

import numpy as np


class MeshCache:
    """blocks: {(x, y, z): chunk}, chunk = positions [t, 3, 3] float32, or (positions, normals) with normals=True.  color=True
    makes a change of a colour word count as a change of the block (for a consumer that colours the vertices with
    sample_color); the chunks themselves carry no colour."""

    def __init__(self, table, normals: bool = False, color: bool = False):
        self.table, self.normals, self.color = table, bool(normals), bool(color)
        self.state = table.changes_state()
        self.blocks = {}

    def update(self, region=None) -> dict:
        """Brings the cache up to the model: {"changed", "removed", "extracted", "triangles"} -- the blocks listed (self-changed or
        halo), the keys dropped, the blocks re-extracted and the triangles they gave."""
        changed, removed = self.table.changes(self.state, region=region, color=self.color,
                                              halo="normals" if self.normals else "mesh")
        for k in removed.cpu().numpy()[:, :3].tolist():
            self.blocks.pop(tuple(k), None)
        n = int(changed.shape[0])
        triangles = 0
        if n:
            pos, nrm, first = self.table.extract_mesh_blocks(changed, normals=self.normals)
            first = first.astype(np.int64)
            triangles = int(first[-1])
            for j, k in enumerate(changed.cpu().numpy()[:, :3].tolist()):
                a, b = int(first[j]), int(first[j + 1])
                self.blocks[tuple(k)] = (pos[a:b].copy(), nrm[a:b].copy()) if self.normals else pos[a:b].copy()
        return {"changed": n, "removed": int(removed.shape[0]), "extracted": n, "triangles": triangles}

    def triangles(self):
        """The cached mesh in ascending key order (deterministic): positions [T, 3, 3], or (positions, normals)."""
        keys = sorted(self.blocks)
        if self.normals:
            parts = [self.blocks[k] for k in keys]
            pos = [p for p, _ in parts] or [np.zeros((0, 3, 3), np.float32)]
            nrm = [q for _, q in parts] or [np.zeros((0, 3, 3), np.float32)]
            return np.concatenate(pos), np.concatenate(nrm)
        return np.concatenate([self.blocks[k] for k in keys] or [np.zeros((0, 3, 3), np.float32)])
