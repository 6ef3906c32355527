"""voxelhashing_demo_amd -- MI355X-native voxel-hashing TSDF fusion path.

The product is libvoxelhash_hip.so (hand-written gfx950 HIP behind the C-ABI in
include/voxelhash.h) plus the host-side mirrors of the reference's
SDF_Hashtable class: C++ (include/SDF_Hashtable.h) and Python (hashtable.py).
"""
from ._lib import (COMPONENT_INSIDE, COMPONENT_NONE, COMPONENT_OUTSIDE, ESDF_FAR, ESDF_MAX_RADIUS, ESDF_NONE, ESDF_UNKNOWN_FREE, ESDF_UNKNOWN_KEEP, ESDF_UNKNOWN_OCCUPIED,  # noqa: F401
                   RAY_HIT, RAY_MISS, RAY_REFUSED, SAMPLE_NEAREST, SAMPLE_TRILINEAR, SEM_PINHOLE, SEM_REFERENCE, STREAM_BOX, STREAM_FOREIGN,  # noqa: F401
                   STREAM_PLACED, STREAM_PRESENT, STREAM_SPHERE, STREAM_UNPLACED, HashTableParams, VoxelHashError, load)
from ._lib import CHANGED_HALO, CHANGED_SELF  # noqa: F401
from .hashtable import ENTRY_DTYPE, RECORD_DTYPE, VOXEL_DTYPE, SDFHashtable, default_params, pinhole_rays, preprocess  # noqa: F401

RAYCAST_FIXED_STEP, RAYCAST_DDA = 0, 1      # vh_set_option(ctx, "raycast_mode", ...), include/voxelhash.h
BAND_RAY, BAND_NORMAL_DDA, BAND_RAY_DDA = 0, 1, 2      # vh_set_option(ctx, "band_mode", ...)
