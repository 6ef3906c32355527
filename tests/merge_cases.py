"""Inputs shared by tests/test_merge_ref_cpu.py and tests/test_gpu_merge.py: the 64x48 synthetic-room frames and parameters of
tests/deintegrate_cases.py (numBuckets = 2^11, voxelSize = 0.04, at most a few hundred source blocks), dst pools of 4096
blocks so that the dilation of the candidate rule fits, the transforms, and ball shells for the CPU tests."""
import math

import numpy as np

import deintegrate_cases as DC
import mesh_models as MM

F = np.float32
W, H = DC.W, DC.H
VS = DC.KW["voxelSize"]
SRC_KW = dict(DC.KW)                                        # pool of 512 blocks
DST_KW = dict(DC.KW, numVoxelBlocks=4096)
SRC_FRAMES, DST_FRAMES = (0, 1), (2,)                       # src is fused from two frames, a dst that holds a model from the third


def rigid(axis, degrees, translation):
    """Rotation about `axis` (Rodrigues, float64) and a translation, as the float32 matrix the library is handed."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    T[:3, 3] = translation
    return T.astype(F)


IDENTITY = np.eye(4, dtype=F)
OBLIQUE = rigid((0.3, 1.0, -0.45), 27.0, (0.113, -0.071, 0.057))          # no axis kept, a translation off the lattice
STEEP = rigid((-0.7, 0.2, 0.6), 63.0, (-0.031, 0.209, 0.147))
HALF_SHIFT = rigid((0, 0, 1), 0.0, (VS / 2, VS / 2, VS / 2))              # every dst voxel in the middle of a src cell
TRANSFORMS = {"identity": IDENTITY, "oblique": OBLIQUE, "half-shift": HALF_SHIFT}
# (name of the transform, vs_d / vs_s, mode) of the GPU cases beyond the first two
REGRID = [("oblique", 0.5, 1), ("oblique", 2.0, 1), ("oblique", 1.0, 0), ("half-shift", 1.0, 1)]


def shell(centre=(3.3, -2.1, 5.7), radius=11.3, seed=5, dead=0.01):
    """A ball_model shell: the blocks of a cube of keys that the sphere's surface comes within a voxel of (a few dozen)."""
    c = np.asarray(centre)
    lo, hi = np.floor((c - radius - 2) / 8).astype(int), np.ceil((c + radius + 2) / 8).astype(int) + 1
    keys, vox = MM.ball_model(MM.cube_keys(lo, hi), centre, radius, seed, dead=dead)
    keep = np.abs(vox["sdf"]).min(1) < 1.0
    return MM.as_model(keys[keep], vox[keep])


def dilation(keys):
    """The keys within one block of the set, the set included."""
    out = set()
    for k in keys:
        for d in MM.NEIGHBOURS + [(0, 0, 0)]:
            out.add((k[0] + d[0], k[1] + d[1], k[2] + d[2]))
    return out


def with_new_blocks(model, keys):
    """The model with a zeroed block for every key it lacks: what the allocation leaves for the update."""
    out = dict(model)
    for k in keys:
        if k not in out:
            out[k] = (np.zeros(512, F), np.zeros(512, F))
    return out
