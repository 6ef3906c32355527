"""Small scenes shared by tests/test_deintegrate_ref_cpu.py and tests/test_gpu_deintegrate.py: 64x48 uint16 sensor images of
the synthetic room from three poses that overlap only partly, with sensor holes, and what goes with them (K^-1, the
projection the library's default would pick, the oracle-side model builder)."""
import numpy as np

from voxelhashing_demo_amd import synth

W, H = 64, 48
# 4 cm voxels: a block spans ~8 pixels at 2 m, a frame allocates well under 512 blocks and no bucket of 2^11 overflows
KW = dict(numBuckets=1 << 11, numVoxelBlocks=512, voxelSize=0.04)
POSES = [synth.yaw_pose(0.0), synth.yaw_pose(8.0, (0.1, 0.0, 0.05)), synth.yaw_pose(-6.0, (-0.05, 0.02, 0.1))]
NOWHERE = synth.yaw_pose(180.0, (0.0, 40.0, 0.0))         # a pose that sees no block of the models built here


def k_inv(width=W, height=H):
    return np.linalg.inv(synth.K_matrix(width, height).astype(np.float64)).astype(np.float32)


def projection(semantics, width=W, height=H):
    """What vh_create installs: K, transposed under REFERENCE semantics."""
    return synth.K_matrix(width, height, transposed=(semantics == 0))


def sensor_image(pose, width=W, height=H, holes=True):
    z = synth.render_room_verts(pose, width, height, synth.room_primitives()).numpy()[..., 2]
    d16 = np.round(z * 5000.0).clip(0, 65535).astype(np.uint16)
    if holes:
        d16[::11, ::5] = 0
    return d16


_FRAMES = {}


def frames(oracle, width=W, height=H):
    """[(pose, d16 [H, W], verts [H, W, 4])] for POSES, computed once per size; treat as read-only."""
    key = (width, height)
    if key not in _FRAMES:
        out = []
        for pose in POSES:
            d16 = sensor_image(pose, width, height)
            out.append((pose, d16, oracle.preprocess(d16, k_inv(width, height))[0]))
        _FRAMES[key] = out
    return _FRAMES[key]


def oracle_table(oracle, semantics, flags=0, **kw):
    p = dict(KW)
    p.update(kw)
    t = oracle.OracleTable(oracle.default_params(**p), W, H, semantics)
    t.set_projection(projection(semantics))
    t.set_integrate_flags(flags)
    return t
