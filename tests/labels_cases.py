"""Label images shared by tests/test_labels_ref_cpu.py and tests/test_gpu_labels.py, for the small room scenes of
tests/deintegrate_cases.py."""
import numpy as np

import deintegrate_cases as DC

POSE_ORDER = (0, 1, 2, 1, 0, 2, 1)          # the seven label calls over the three fused frames
VOTE_MAX = 3


def image(i, width=DC.W, height=DC.H, noise=0.3):
    """The label image of call i: 16-pixel patches of the labels 1..3, different per call, with `noise` of the pixels redrawn
    from {0, 1, 2, 3} (0: not labelled)."""
    rng = np.random.default_rng(200 + i)
    patches = rng.integers(1, 4, (-(-height // 16), -(-width // 16)))
    img = np.kron(patches, np.ones((16, 16), np.int64))[:height, :width]
    redrawn = rng.random((height, width)) < noise
    return np.where(redrawn, rng.integers(0, 4, (height, width)), img).astype(np.uint16)


def halves(width=DC.W, height=DC.H):
    """Left half 7, right half 9."""
    img = np.full((height, width), 9, np.uint16)
    img[:, :width // 2] = 7
    return img
