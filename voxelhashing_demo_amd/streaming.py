"""Block streaming policy on the host (Niessner et al. 2013, section 5): the model may be larger than the GPU's
block pool.  Blocks that leave an active sphere around the camera move into a host store and their pool slots are freed
(SDFHashtable.stream_out); stored blocks move back when the camera returns (SDFHashtable.stream_in).

The selection rule is the library's (include/voxelhash.h, "block streaming"), restated here in numpy float32 so that the store
picks exactly the blocks the GPU would: per axis x_a = ((float)(8 * key_a) + 3.5f) * voxelSize - centre_a,
d2 = (x_0 * x_0 + x_1 * x_1) + x_2 * x_2, inside iff d2 <= radius * radius, every operation rounded on its own.
"""
from __future__ import annotations

import numpy as np

from ._lib import STREAM_BOX, STREAM_PLACED, STREAM_SPHERE

F = np.float32


def box(lo, hi, invert: bool = False) -> dict:
    """The blocks with lo <= key < hi on every axis (invert: all the others)."""
    return {"kind": STREAM_BOX, "invert": bool(invert), "lo": tuple(int(v) for v in lo), "hi": tuple(int(v) for v in hi)}


def sphere(centre, radius: float, invert: bool = False) -> dict:
    """The blocks whose centre lies within `radius` metres of `centre` (invert: all the others)."""
    return {"kind": STREAM_SPHERE, "invert": bool(invert), "centre": tuple(float(v) for v in centre), "radius": float(radius)}


def selected(keys, region: dict, voxel_size: float) -> np.ndarray:
    """bool [n]: which of the block keys int32 [n, 3] `region` selects -- the library's rule, bit for bit."""
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    if region["kind"] == STREAM_BOX:
        lo, hi = np.asarray(region["lo"], np.int64), np.asarray(region["hi"], np.int64)
        inside = np.all((keys >= lo) & (keys < hi), axis=1)
    else:
        vs, c = F(voxel_size), np.asarray(region["centre"], F)
        x = ((keys * np.int32(8)).astype(F) + F(3.5)) * vs - c             # (one rounding per operation: float32 arrays)
        sq = x * x
        d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        r = F(region["radius"])
        inside = d2 <= r * r
    return inside != bool(region.get("invert", False))


class BlockStore:
    """A host store {key: (voxels [512] {sdf, weight}, colours [512] uint32 or None)} with the paper's hysteresis policy.

    It talks to the table only through table.stream_out(region) and table.stream_in(chunk), so anything with those two methods
    can stand in for an SDFHashtable.

    The store does not fuse: a key has one record.  Choose r_out beyond the sensor's depth range -- a block the camera still sees
    outside r_out is allocated again by the next frame, and when that new block streams out it REPLACES the stored record of its
    key; a stored block whose key the table has allocated again comes back PRESENT and stays in the store (fusing the two is
    vh_import_view + vh_merge)."""

    def __init__(self, voxel_size: float):
        self.voxel_size = float(voxel_size)
        self._blocks = {}

    def __len__(self) -> int:
        return len(self._blocks)

    def __contains__(self, key) -> bool:
        return tuple(int(v) for v in key) in self._blocks

    def keys(self):
        return list(self._blocks)

    def block(self, key):
        return self._blocks[tuple(int(v) for v in key)]

    def _take(self, chunk) -> int:
        cols = chunk.get("colors")
        for i, k in enumerate(np.asarray(chunk["keys"]).reshape(-1, 3).tolist()):
            # (a block the table still held under a key the store kept -- PRESENT at an earlier stream-in -- is the newer one)
            self._blocks[tuple(k)] = (np.array(chunk["voxels"][i]), None if cols is None else np.array(cols[i]))
        return len(chunk["keys"])

    def _give(self, table, keys) -> dict:
        """Streams the stored blocks `keys` in; only what comes back PLACED leaves the store."""
        none = {"placed": 0, "present": 0, "unplaced": 0, "foreign": 0, "rounds": 0}
        if not keys:
            return none
        vox = np.stack([self._blocks[k][0] for k in keys])
        have = [self._blocks[k][1] is not None for k in keys]
        cols = None
        if any(have):
            cols = np.stack([self._blocks[k][1] if h else np.zeros(512, np.uint32) for k, h in zip(keys, have)])
        st = table.stream_in({"keys": np.asarray(keys, np.int32).reshape(-1, 3), "voxels": vox, "colors": cols})
        for k, s in zip(keys, np.asarray(st["status"]).tolist()):
            if s == STREAM_PLACED:
                del self._blocks[k]
        return {n: int(st[n]) for n in none}

    def update(self, table, centre, r_in: float, r_out: float) -> dict:
        """One step of the policy around `centre` (world metres): every block of the table outside the sphere of r_out moves
        into the store, then every stored block inside the sphere of r_in moves back (r_in <= r_out: a block between the two
        stays where it is, so a camera that dithers does not make blocks bounce).  Blocks the table could not take back
        (PRESENT, UNPLACED, FOREIGN) stay in the store.  Returns what moved: {"out", "in", "present", "unplaced", "foreign",
        "stored"}."""
        if not (np.isfinite(r_in) and np.isfinite(r_out) and 0.0 <= r_in <= r_out):
            raise ValueError("update: 0 <= r_in <= r_out is required")
        moved_out = self._take(table.stream_out(sphere(centre, r_out, invert=True)))
        keys = list(self._blocks)
        back = []
        if keys:
            inside = selected(np.asarray(keys, np.int32), sphere(centre, r_in), self.voxel_size)
            back = [k for k, i in zip(keys, inside.tolist()) if i]
        st = self._give(table, back)
        return {"out": moved_out, "in": st["placed"], "present": st["present"], "unplaced": st["unplaced"],
                "foreign": st["foreign"], "stored": len(self)}

    def restore_all(self, table) -> dict:
        """Streams every stored block back in; returns the totals of the call and what stayed behind ("stored")."""
        st = self._give(table, list(self._blocks))
        st["stored"] = len(self)
        return st
