"""Inputs shared by tests/test_gpu_stream.py and tests/test_gpu_stream_cpp.py: the coloured two-frame model of
tests/merge_color_cases.py (64x48 frames, 2^11 buckets, 512 blocks, 4 cm voxels: tests/deintegrate_cases.py) and regions cut
through the middle of whatever blocks it holds, so that many go and many stay."""
import numpy as np

import deintegrate_cases as DC
import merge_color_cases as CC
import stream_ref as S

F = np.float32
U = np.uint32
VS = DC.KW["voxelSize"]
EVERYTHING = S.box((-(1 << 31),) * 3, ((1 << 31) - 1,) * 3)


def coloured(vh, torch, oracle, sem=1, bucket_range=None, **kw):
    """The model of frames 0 and 1, each coloured twice (CC.SRC_COLORS)."""
    gt = CC.table(vh, DC.KW, sem, bucket_range=bucket_range, **kw)
    CC.fuse(torch, gt, oracle, CC.SRC_COLORS)
    return gt


def live_keys(table):
    return table["pos"][table["ptr"] != -1]


def middle_sphere(keys, invert=False):
    """A sphere around the mean block centre with the median distance as radius: about half of `keys` inside."""
    centres = (8.0 * np.asarray(keys, np.float64) + 3.5) * VS
    c = centres.mean(axis=0).astype(F)
    r = F(np.median(np.linalg.norm(centres - c, axis=1)))
    return S.sphere(tuple(float(v) for v in c), float(r), invert)


def middle_box(keys):
    """The blocks below the median x key."""
    big = 1 << 31
    return S.box((-big, -big, -big), (int(np.median(np.asarray(keys)[:, 0])), big - 1, big - 1))


def regions(keys):
    return {"box": middle_box(keys), "sphere": middle_sphere(keys), "outside": middle_sphere(keys, invert=True)}


def chunk_model(chunk):
    """{key: (sdf, weight, colour)} of what stream_out returned."""
    cols = chunk["colors"]
    return {tuple(k): (chunk["voxels"]["sdf"][i], chunk["voxels"]["weight"][i], np.zeros(512, U) if cols is None else cols[i])
            for i, k in enumerate(chunk["keys"].tolist())}
