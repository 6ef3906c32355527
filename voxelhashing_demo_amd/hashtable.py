"""Host-side mirror of the reference's SDF_Hashtable class (SDF_Hashtable.h:24-42)
for Python callers: same entry points (integrate, plus raycast standing in for
SDFRenderer::render), every call going straight through the C-ABI of
libvoxelhash_hip.so.  torch is used only as the owner of device buffers and of
the current stream; none of the path's arithmetic is done in torch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

ENTRY_DTYPE = np.dtype([("pos", "<i4", (3,)), ("ptr", "<i4"), ("offset", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<f4"), ("weight", "<f4")])
RECORD_DTYPE = np.dtype([("pos", "<i4", (3,)), ("reserved", "<i4"), ("voxels", VOXEL_DTYPE, (512,))])    # vh_view_record, 4112 bytes


def default_params(**overrides) -> L.HashTableParams:
    """common.h:39-50 as copied by SDF_Hashtable.cpp:62-73, with overrides."""
    p = L.HashTableParams()
    L.load().vh_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _dev_ptr(t) -> int:
    """Device address of a torch CUDA tensor (or a raw int address)."""
    if isinstance(t, int):
        return t
    if t is None:
        return 0
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("expected a contiguous CUDA tensor")
    return t.data_ptr()


def _pose16(pose):
    a = np.ascontiguousarray(np.asarray(pose, dtype=np.float32).reshape(16))
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def preprocess(depth_u16, k_inv, positions, normals, stream=None):
    """preProcess (CameraTrackingUtils.cu:115-120) on the GPU: uint16 depth [H, W] -> float4 vertex
    and normal maps [H, W, 4] (device tensors, written in place)."""
    H, W = depth_u16.shape
    k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
    handle = 0 if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
    L.check(L.load().vh_preprocess(_dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)), W, H,
                                   _dev_ptr(positions), _dev_ptr(normals), C.c_void_p(handle)), "vh_preprocess")
    return positions, normals


def pinhole_rays(pose, fx, fy, cx, cy, W, H, t_min, t_max):
    """The rays of vh_raycast's view as vh_cast_rays takes them: [H * W, 8] float32 (origin, t_min, direction, t_max), row-major
    over the image, with the raycast's own rounding -- dx = (u - cx) / fx, dy = (v - cy) / fy, D_a = (T[a,0] * dx + T[a,1] * dy)
    + T[a,2], origin = the pose's translation -- in numpy float32, every operation rounded on its own."""
    F = np.float32
    T = np.asarray(pose, F).reshape(4, 4)
    v, u = np.divmod(np.arange(int(W) * int(H)), int(W))
    dx, dy = (u.astype(F) - F(cx)) / F(fx), (v.astype(F) - F(cy)) / F(fy)
    rays = np.empty((len(u), 8), F)
    for a in range(3):
        rays[:, a] = T[a, 3]
        rays[:, 4 + a] = (T[a, 0] * dx + T[a, 1] * dy) + T[a, 2]
    rays[:, 3], rays[:, 7] = F(t_min), F(t_max)
    return rays


class SDFHashtable:
    """One voxel-hash table on one GPU.

    integrate(pose, verts, normals) == SDF_Hashtable::integrate (SDF_Hashtable.cpp:11-40);
    raycast(pose) stands in for SDFRenderer::render (SDFRenderer.cpp:210-255).
    """

    def __init__(self, params: L.HashTableParams | None = None, width: int = 640, height: int = 480,
                 semantics: int = L.SEM_REFERENCE, device: int = -1, bucket_range=None, stream=None):
        self._lib = L.load()
        self.params = params if params is not None else default_params()
        self.width, self.height, self.semantics = width, height, semantics
        cfg = L.Config(self.params, width, height, semantics, device)
        self._device = device
        h = C.c_void_p()
        if bucket_range is None:
            L.check(self._lib.vh_create(C.byref(cfg), C.byref(h)), "vh_create")
            self.bucket_range = (0, self.params.numBuckets)
        else:
            lo, hi = bucket_range
            L.check(self._lib.vh_create_shard(C.byref(cfg), lo, hi, C.byref(h)), "vh_create_shard")
            self.bucket_range = (lo, hi)
        self._h = h
        self.stream_handle = 0                  # raw hipStream_t the context enqueues on (0 = default stream)
        if stream is not None:
            self.set_stream(stream)

    @classmethod
    def borrowed(cls, handle, params, width, height, semantics, bucket_range):
        """A view of a context somebody else owns (a vh_dist's shard): every query and option works, close() leaves it."""
        t = cls.__new__(cls)
        t._lib = L.load()
        t.params, t.width, t.height, t.semantics = params, width, height, semantics
        t.bucket_range = tuple(bucket_range)
        t._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        t._borrowed = True
        t.stream_handle = 0
        return t

    # ---- lifecycle ----
    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._lib.vh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """`stream`: a torch.cuda.Stream, or a raw hipStream_t address."""
        handle = stream if isinstance(stream, int) else stream.cuda_stream
        L.check(self._lib.vh_set_stream(self._h, C.c_void_p(handle)), "vh_set_stream")
        self.stream_handle = handle

    def set_projection(self, m):
        a = np.ascontiguousarray(np.asarray(m, np.float32).reshape(9))
        L.check(self._lib.vh_set_projection(self._h, a.ctypes.data_as(C.POINTER(C.c_float))), "vh_set_projection")

    def set_alloc_band(self, band_metres: float):
        """Opt-in truncation-band allocation; 0 = the reference's surface-block-only allocation."""
        L.check(self._lib.vh_set_alloc_band(self._h, float(band_metres)), "vh_set_alloc_band")

    def set_raycast_intrinsics(self, fx, fy, cx, cy):
        L.check(self._lib.vh_set_raycast_intrinsics(self._h, fx, fy, cx, cy), "vh_set_raycast_intrinsics")

    # ---- the hot path ----
    def integrate(self, pose, verts, normals=None):
        """Asynchronous: pose -> lock epoch -> allocBlocks -> flatten -> integrateDepthMap."""
        _, pp = _pose16(pose)
        L.check(self._lib.vh_integrate(self._h, pp, _dev_ptr(verts), _dev_ptr(normals)), "vh_integrate")

    def integrate_depth(self, pose, depth_u16, k_inv):
        """The frame straight from the uint16 sensor image [H, W] (== preprocess + integrate)."""
        _, pp = _pose16(pose)
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_integrate_depth(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float))),
                "vh_integrate_depth")

    # ---- taking a frame back out ----
    def _check_verts(self, verts, what):
        if not isinstance(verts, int):
            import torch
            if verts.dtype != torch.float32:
                raise ValueError(f"{what}: the vertex map must be float32")
            if verts.numel() != self.width * self.height * 4:
                raise ValueError(f"{what}: the vertex map must hold height * width float4 vertices")
            if not verts.is_cuda:
                raise ValueError(f"{what}: the vertex map must be a CUDA tensor")

    def _check_depth_u16(self, depth_u16, what):
        if not isinstance(depth_u16, int):
            import torch
            if depth_u16.dtype != torch.uint16:
                raise ValueError(f"{what}: the sensor image must be uint16")
            if depth_u16.numel() != self.width * self.height:
                raise ValueError(f"{what}: the sensor image must hold height * width pixels")
            if not depth_u16.is_cuda:
                raise ValueError(f"{what}: the sensor image must be a CUDA tensor")

    def deintegrate(self, pose, verts):
        """Asynchronous: the TSDF update of integrate(pose, verts) run backwards over the blocks `pose` sees.  The exact inverse
        only below the weight cap and with the frame's options, up to fp32 rounding; garbage_collect() directly afterwards
        frees the blocks the removal emptied."""
        _, pp = _pose16(pose)
        self._check_verts(verts, "deintegrate")
        L.check(self._lib.vh_deintegrate(self._h, pp, _dev_ptr(verts)), "vh_deintegrate")

    def deintegrate_depth(self, pose, depth_u16, k_inv):
        """The same straight from the uint16 sensor image [H, W] (== preprocess + deintegrate)."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "deintegrate_depth")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_deintegrate_depth(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float))),
                "vh_deintegrate_depth")

    def reintegrate_depth(self, old_pose, new_pose, depth_u16, k_inv):
        """deintegrate_depth(old_pose) + integrate_depth(new_pose): a frame moved to its corrected pose."""
        _, po = _pose16(old_pose)
        _, pn = _pose16(new_pose)
        self._check_depth_u16(depth_u16, "reintegrate_depth")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_reintegrate_depth(self._h, po, pn, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float))),
                "vh_reintegrate_depth")

    # ---- one model into another ----
    def merge(self, src, src_to_dst, mode: int = L.SAMPLE_TRILINEAR, colors: bool = False, color_weight_max: int = 255) -> dict:
        """vh_merge: the model of `src` (another SDFHashtable on this device) fused into this one under the rigid 4x4
        src_to_dst (src world metres -> this model's).  Voxel sizes may differ.  Synchronises this context's stream; src is only
        read.  Returns vh_merge_stats as a dict; garbage_collect() directly afterwards frees the candidate blocks that stayed
        empty.  colors=True is vh_merge_color: the same call with src's colour carried along in the same launch
        (color_weight_max: 1..255, the cap of the merged sample counts); a src without colour gives exactly the plain merge."""
        if not isinstance(src, SDFHashtable):
            raise TypeError("merge: src must be an SDFHashtable")
        _, pp = _pose16(src_to_dst)
        st = L.MergeStats()
        if colors:
            L.check(self._lib.vh_merge_color(self._h, src._h, pp, int(mode), int(color_weight_max), C.byref(st)), "vh_merge_color")
        else:
            L.check(self._lib.vh_merge(self._h, src._h, pp, int(mode), C.byref(st)), "vh_merge")
        return st.as_dict()

    # ---- the model in colour ----
    def _check_rgba(self, rgba, what):
        if not isinstance(rgba, int):
            if rgba.element_size() != 4 or rgba.is_floating_point():
                raise ValueError(f"{what}: the colour image must hold one 32-bit word per pixel (r | g << 8 | b << 16)")
            if rgba.numel() != self.width * self.height:
                raise ValueError(f"{what}: the colour image must hold height * width pixels")
            if not rgba.is_cuda:
                raise ValueError(f"{what}: the colour image must be a CUDA tensor")

    def integrate_color(self, pose, depth_u16, k_inv, rgba, band: float, weight_max: int = 255):
        """Asynchronous: the colour image `rgba` [H, W] (one word per pixel, registered to the uint16 depth image) averaged
        into the voxels within `band` metres of the surface, over the blocks `pose` sees.  weight_max: 1..255, the window of
        the running average; 0 only sweeps the colour of voxels that hold nothing (the pairing after a de-integration).
        The first call allocates the colour volume."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "integrate_color")
        self._check_rgba(rgba, "integrate_color")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_integrate_color(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                             _dev_ptr(rgba), float(band), int(weight_max)), "vh_integrate_color")

    def integrate_color_map(self, pose, verts, rgba, band: float, weight_max: int = 255):
        """The same with the depth taken from the .z of a float4 vertex map [H, W, 4]."""
        _, pp = _pose16(pose)
        self._check_verts(verts, "integrate_color_map")
        self._check_rgba(rgba, "integrate_color_map")
        L.check(self._lib.vh_integrate_color_map(self._h, pp, _dev_ptr(verts), _dev_ptr(rgba), float(band), int(weight_max)),
                "vh_integrate_color_map")

    def integrate_depth_color(self, pose, depth_u16, k_inv, rgba, band: float, weight_max: int = 255):
        """One RGB-D frame: integrate_depth followed by integrate_color."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "integrate_depth_color")
        self._check_rgba(rgba, "integrate_depth_color")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_integrate_depth_color(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                   _dev_ptr(rgba), float(band), int(weight_max)), "vh_integrate_depth_color")

    # ---- colour through de-integration and saved models ----
    def deintegrate_color(self, pose, depth_u16, k_inv, rgba, band: float):
        """Asynchronous: the colour sample integrate_color(pose, ...) added taken back out of the running averages (the exact
        inverse only below the colour cap, up to byte rounding).  Call it before the frame's deintegrate_depth."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "deintegrate_color")
        self._check_rgba(rgba, "deintegrate_color")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_deintegrate_color(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                               _dev_ptr(rgba), float(band)), "vh_deintegrate_color")

    def deintegrate_depth_color(self, pose, depth_u16, k_inv, rgba, band: float):
        """One RGB-D frame taken back out: deintegrate_color, deintegrate_depth, then the sweep of the voxels that emptied."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "deintegrate_depth_color")
        self._check_rgba(rgba, "deintegrate_depth_color")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_deintegrate_depth_color(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                     _dev_ptr(rgba), float(band)), "vh_deintegrate_depth_color")

    def reintegrate_depth_color(self, old_pose, new_pose, depth_u16, k_inv, rgba, band: float, weight_max: int = 255):
        """deintegrate_depth_color(old_pose) + integrate_depth_color(new_pose): an RGB-D frame moved to its corrected pose."""
        _, po = _pose16(old_pose)
        _, pn = _pose16(new_pose)
        self._check_depth_u16(depth_u16, "reintegrate_depth_color")
        self._check_rgba(rgba, "reintegrate_depth_color")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_reintegrate_depth_color(self._h, po, pn, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                                     _dev_ptr(rgba), float(band), int(weight_max)), "vh_reintegrate_depth_color")

    def save_color(self, path: str):
        """The colour words of the allocated blocks as a file beside a snapshot (save_snapshot + save_color)."""
        L.check(self._lib.vh_save_color(self._h, str(path).encode()), "vh_save_color")

    def load_color(self, path: str):
        """Restores save_color's file into the model as it is now: call it after load_snapshot.  A file that does not match
        the model's blocks is refused and nothing changes."""
        L.check(self._lib.vh_load_color(self._h, str(path).encode()), "vh_load_color")

    def has_color(self) -> bool:
        return bool(self._lib.vh_has_color(self._h))

    def clear_color(self):
        L.check(self._lib.vh_clear_color(self._h), "vh_clear_color")

    def color_volume(self) -> np.ndarray:
        """The colour words of the whole volume (uint32, r | g << 8 | b << 16 | count << 24; 0 = no colour), indexed like
        sdf_blocks().  Raises when the context has no colour volume."""
        out = np.empty(self.params.numVoxelBlocks * 512, np.uint32)
        L.check(self._lib.vh_download_color(self._h, 0, out.ctypes.data_as(C.c_void_p), out.size), "vh_download_color")
        return out

    def block_colors(self, ptr: int) -> np.ndarray:
        """The 512 colour words of the block at voxel index `ptr` (an entry's ptr)."""
        out = np.empty(512, np.uint32)
        L.check(self._lib.vh_download_color(self._h, int(ptr), out.ctypes.data_as(C.c_void_p), out.size), "vh_download_color")
        return out

    def sample_color_into(self, points, rgba, mode: int = L.SAMPLE_TRILINEAR, n: int = None):
        """vh_sample_color into a caller-owned device buffer: points [n, 3] float32 (world metres), rgba [n] 32-bit words
        (r | g << 8 | b << 16 | 0xFF << 24; 0 = no colour).  Asynchronous on the context's stream."""
        n = int(points.shape[0]) if n is None else int(n)
        L.check(self._lib.vh_sample_color(self._h, int(mode), n, _dev_ptr(points), _dev_ptr(rgba)), "vh_sample_color")
        return rgba

    def sample_color(self, points, mode: int = L.SAMPLE_TRILINEAR):
        """The colour at world points [n, 3] (float32 CUDA tensor) as a uint32 CUDA tensor [n]."""
        import torch
        rgba = torch.empty((int(points.shape[0]),), dtype=torch.uint32, device=points.device)
        return self.sample_color_into(points, rgba, mode)

    def sample_color_map_into(self, pose, points4, rgba, mode: int = L.SAMPLE_TRILINEAR, n: int = None):
        """vh_sample_color_map: camera-frame float4 points [n, 4] (a vertex map; .z == 0: no point) moved by `pose`."""
        _, pp = _pose16(pose)
        n = int(points4.numel() // 4) if n is None else int(n)
        L.check(self._lib.vh_sample_color_map(self._h, int(mode), pp, n, _dev_ptr(points4), _dev_ptr(rgba)),
                "vh_sample_color_map")
        return rgba

    def render_color(self, pose, t_min: float = 0.1, t_max: float = 5.0, mode: int = L.SAMPLE_TRILINEAR):
        """The model seen from `pose` in colour (vh_raycast_color): (depth [H, W], vertices [H, W, 4], normals [H, W, 4],
        rgba [H, W] uint32) as CUDA tensors; a pixel without a hit or without colour is 0."""
        import torch
        _, pp = _pose16(pose)
        with torch.cuda.device(self.device_index()):
            depth = torch.empty((self.height, self.width), dtype=torch.float32, device="cuda")
            verts = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
            nrm = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
            rgba = torch.empty((self.height, self.width), dtype=torch.uint32, device="cuda")
        L.check(self._lib.vh_raycast_color(self._h, pp, t_min, t_max, _dev_ptr(depth), _dev_ptr(verts), _dev_ptr(nrm), int(mode),
                                           _dev_ptr(rgba)), "vh_raycast_color")
        return depth, verts, nrm, rgba

    # ---- the model with labels ----
    def _check_label_image(self, labels_u16, what):
        if not isinstance(labels_u16, int):
            if labels_u16.element_size() != 2 or labels_u16.is_floating_point():
                raise ValueError(f"{what}: the label image must hold one 16-bit label per pixel (0: not labelled)")
            if labels_u16.numel() != self.width * self.height:
                raise ValueError(f"{what}: the label image must hold height * width pixels")
            if not labels_u16.is_cuda:
                raise ValueError(f"{what}: the label image must be a CUDA tensor")

    def integrate_labels(self, pose, depth_u16, k_inv, labels_u16, band: float, vote_max: int = 65535):
        """Asynchronous: the label image `labels_u16` [H, W] (uint16 or int16 storage, registered to the uint16 depth image; 0 =
        not labelled) cast as one Boyer-Moore vote into every voxel within `band` metres of the surface, over the blocks `pose`
        sees.  vote_max: 1..65535, the cap of a voxel's vote count; 0 only sweeps the labels of voxels that hold nothing (the
        pairing after a de-integration).  The first call allocates the label volume."""
        _, pp = _pose16(pose)
        self._check_depth_u16(depth_u16, "integrate_labels")
        self._check_label_image(labels_u16, "integrate_labels")
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_integrate_labels(self._h, pp, _dev_ptr(depth_u16), k.ctypes.data_as(C.POINTER(C.c_float)),
                                              _dev_ptr(labels_u16), float(band), int(vote_max)), "vh_integrate_labels")

    def integrate_labels_map(self, pose, verts, labels_u16, band: float, vote_max: int = 65535):
        """integrate_labels with the depth taken from the .z of a float4 vertex map [H, W, 4]."""
        _, pp = _pose16(pose)
        self._check_verts(verts, "integrate_labels_map")
        self._check_label_image(labels_u16, "integrate_labels_map")
        L.check(self._lib.vh_integrate_labels_map(self._h, pp, _dev_ptr(verts), _dev_ptr(labels_u16), float(band), int(vote_max)),
                "vh_integrate_labels_map")

    def has_labels(self) -> bool:
        return bool(self._lib.vh_has_labels(self._h))

    def clear_labels(self):
        L.check(self._lib.vh_clear_labels(self._h), "vh_clear_labels")

    def label_volume(self) -> np.ndarray:
        """The label words of the whole volume (uint32, label | votes << 16; 0 = no label), indexed like sdf_blocks().  Raises
        when the context has no label volume."""
        out = np.empty(self.params.numVoxelBlocks * 512, np.uint32)
        L.check(self._lib.vh_download_labels(self._h, 0, out.ctypes.data_as(C.c_void_p), out.size), "vh_download_labels")
        return out

    def sample_labels_into(self, points, words, min_votes: int = 1, n: int = None):
        """vh_sample_labels into a caller-owned device buffer: points [n, 3] float32 (world metres), words [n] 32-bit words
        (label | votes << 16 of the nearest voxel; 0 = no label, or fewer than min_votes votes).  Asynchronous."""
        n = int(points.shape[0]) if n is None else int(n)
        L.check(self._lib.vh_sample_labels(self._h, n, _dev_ptr(points), int(min_votes), _dev_ptr(words)), "vh_sample_labels")
        return words

    def sample_labels(self, points, min_votes: int = 1):
        """The label words at world points [n, 3] (float32 CUDA tensor) as a uint32 CUDA tensor [n]; word & 0xFFFF is the label."""
        import torch
        words = torch.empty((int(points.shape[0]),), dtype=torch.uint32, device=points.device)
        return self.sample_labels_into(points, words, min_votes)

    def sample_labels_map_into(self, pose, points4, words, min_votes: int = 1, n: int = None):
        """vh_sample_labels_map: camera-frame float4 points [n, 4] (a vertex map; .z == 0: no point) moved by `pose`."""
        _, pp = _pose16(pose)
        n = int(points4.numel() // 4) if n is None else int(n)
        L.check(self._lib.vh_sample_labels_map(self._h, pp, n, _dev_ptr(points4), int(min_votes), _dev_ptr(words)),
                "vh_sample_labels_map")
        return words

    def render_labels(self, pose, t_min: float = 0.1, t_max: float = 5.0, min_votes: int = 1):
        """The model seen from `pose` with its labels (vh_raycast_labels): (depth [H, W], vertices [H, W, 4], normals [H, W, 4],
        words [H, W] uint32) as CUDA tensors; a pixel without a hit or without a label is 0."""
        import torch
        _, pp = _pose16(pose)
        with torch.cuda.device(self.device_index()):
            depth = torch.empty((self.height, self.width), dtype=torch.float32, device="cuda")
            verts = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
            nrm = torch.empty((self.height, self.width, 4), dtype=torch.float32, device="cuda")
            words = torch.empty((self.height, self.width), dtype=torch.uint32, device="cuda")
        L.check(self._lib.vh_raycast_labels(self._h, pp, t_min, t_max, _dev_ptr(depth), _dev_ptr(verts), _dev_ptr(nrm),
                                            int(min_votes), _dev_ptr(words)), "vh_raycast_labels")
        return depth, verts, nrm, words

    def label_counts_into(self, counts, n_bins: int, region=None, min_votes: int = 1):
        """vh_label_counts into a caller-owned device buffer of n_bins 32-bit words.  Asynchronous."""
        if not isinstance(counts, int) and counts is not None and (counts.element_size() != 4 or counts.numel() < int(n_bins)):
            raise ValueError("label_counts_into: counts must hold n_bins 32-bit words")
        L.check(self._lib.vh_label_counts(self._h, self._mesh_region(region), int(min_votes), int(n_bins), _dev_ptr(counts)),
                "vh_label_counts")
        return counts

    def label_counts(self, n_bins: int, region=None, min_votes: int = 1):
        """The valid voxels of `region` (None: the whole model) per label as a uint32 CUDA tensor [n_bins]: bin l for
        1 <= l < n_bins, bin 0 everything else (unlabelled, fewer than min_votes votes, a label >= n_bins).  Asynchronous."""
        import torch
        if not 1 <= int(n_bins) <= 65536:
            raise ValueError("label_counts: n_bins must be 1..65536")
        with torch.cuda.device(self.device_index()):
            counts = torch.empty((int(n_bins),), dtype=torch.uint32, device="cuda")
        return self.label_counts_into(counts, n_bins, region, min_votes)

    def remove_label(self, label: int, min_votes: int = 1, region=None) -> dict:
        """vh_remove_label: every voxel that carries `label` with at least min_votes votes is cleared out of the volume (voxel
        {0, 0}, colour 0, label 0), and the blocks that emptied are freed.  Returns the stats as a dict.  Synchronises."""
        st = L.LabelStats()
        L.check(self._lib.vh_remove_label(self._h, self._mesh_region(region), int(label), int(min_votes), C.byref(st)),
                "vh_remove_label")
        return st.as_dict()

    def integrate_batch(self, poses, verts_list, normals_list=None):
        """len(poses) frames in len(poses) + 1 launches (pipelined frames, flushed at the end); equals
        integrate() frame by frame."""
        n = len(poses)
        p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, 16))
        v = (C.c_void_p * n)(*[_dev_ptr(t) for t in verts_list])
        nn = None if normals_list is None else (C.c_void_p * n)(*[_dev_ptr(t) for t in normals_list])
        L.check(self._lib.vh_integrate_batch(self._h, n, p.ctypes.data_as(C.POINTER(C.c_float)), v, nn), "vh_integrate_batch")

    def integrate_depth_batch(self, poses, depth_list, k_inv):
        n = len(poses)
        p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, 16))
        d = (C.c_void_p * n)(*[_dev_ptr(t) for t in depth_list])
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_integrate_depth_batch(self._h, n, p.ctypes.data_as(C.POINTER(C.c_float)), d,
                                                   k.ctypes.data_as(C.POINTER(C.c_float))), "vh_integrate_depth_batch")

    def flush(self):
        """Launch the pending half of the last pipelined frame (option "pipeline")."""
        L.check(self._lib.vh_flush(self._h), "vh_flush")

    def raycast(self, pose, out, t_min: float = 0.1, t_max: float = 5.0):
        _, pp = _pose16(pose)
        L.check(self._lib.vh_raycast(self._h, pp, t_min, t_max, _dev_ptr(out)), "vh_raycast")
        return out

    def raycast_normals(self, pose, out, normals, t_min: float = 0.1, t_max: float = 5.0):
        """The DDA raycast with the camera-frame normal map [H, W, 4] of the hits written by the same pass."""
        _, pp = _pose16(pose)
        L.check(self._lib.vh_raycast_normals(self._h, pp, t_min, t_max, _dev_ptr(out), _dev_ptr(normals)),
                "vh_raycast_normals")
        return out, normals

    def set_raycast_mode(self, mode: int):
        """RAYCAST_DDA (default) / RAYCAST_FIXED_STEP."""
        self.set_option("raycast_mode", int(mode))

    def raycast_maps(self, pose, depth, vertices, normals, t_min: float = 0.1, t_max: float = 5.0):
        """raycast + camera-frame vertex and normal maps of the same view (an ICP target)."""
        _, pp = _pose16(pose)
        L.check(self._lib.vh_raycast_maps(self._h, pp, t_min, t_max, _dev_ptr(depth), _dev_ptr(vertices),
                                          _dev_ptr(normals)), "vh_raycast_maps")
        return depth, vertices, normals

    def render_blocks(self, pose, front, back, t_min: float = 0.1, t_max: float = 5.0):
        """Block silhouettes (SDFRenderer::drawToFrontAndBack): nearest front / farthest back cube face per pixel."""
        _, pp = _pose16(pose)
        L.check(self._lib.vh_render_blocks(self._h, pp, t_min, t_max, _dev_ptr(front), _dev_ptr(back)), "vh_render_blocks")
        return front, back

    # ---- deletion / garbage collection ----
    def delete_blocks(self, keys, n: int = None):
        """keys: device int32 [n, 4] = {x, y, z, _}."""
        n = int(keys.shape[0]) if n is None else int(n)
        L.check(self._lib.vh_delete_blocks(self._h, _dev_ptr(keys), n), "vh_delete_blocks")

    def garbage_collect(self, sdf_threshold: float):
        L.check(self._lib.vh_garbage_collect(self._h, float(sdf_threshold)), "vh_garbage_collect")

    # ---- block streaming ----
    @staticmethod
    def _stream_region(region):
        """region: streaming.box(...) / streaming.sphere(...) -- a dict {kind, invert, lo, hi, centre, radius}."""
        r = L.StreamRegion()
        r.kind, r.invert = int(region["kind"]), int(bool(region.get("invert", False)))
        r.block_lo[:] = [int(v) for v in region.get("lo", (0, 0, 0))]
        r.block_hi[:] = [int(v) for v in region.get("hi", (0, 0, 0))]
        r.centre[:] = [float(v) for v in region.get("centre", (0.0, 0.0, 0.0))]
        r.radius = float(region.get("radius", 0.0))
        return r

    def stream_out_into(self, region, capacity: int, records, colors=None):
        """vh_stream_out into caller-owned device buffers: records uint8 [capacity, 4112] (vh_view_record), colors uint32
        [capacity, 512] or None -- then THE COLOUR OF THE REMOVED BLOCKS IS DROPPED.  Returns (selected, written): the allocated
        blocks the region holds and the first `written` = min(selected, capacity) of them in entry order, which have left the
        model.  capacity 0 with None buffers only counts.  Synchronises."""
        sel, wr = C.c_uint64(), C.c_uint64()
        r = self._stream_region(region)
        L.check(self._lib.vh_stream_out(self._h, C.byref(r), int(capacity), _dev_ptr(records), _dev_ptr(colors), C.byref(sel),
                                        C.byref(wr)), "vh_stream_out")
        return int(sel.value), int(wr.value)

    def stream_in_from(self, records, n: int = None, colors=None, status=None) -> dict:
        """vh_stream_in from device buffers: records uint8 [n, 4112], colors uint32 [n, 512] or None, status int32 [n] or None
        (receives STREAM_PLACED / PRESENT / UNPLACED / FOREIGN per record).  Returns vh_stream_stats as a dict.  Synchronises."""
        n = int(records.shape[0]) if n is None else int(n)
        st = L.StreamStats()
        L.check(self._lib.vh_stream_in(self._h, n, _dev_ptr(records), _dev_ptr(colors), _dev_ptr(status), C.byref(st)), "vh_stream_in")
        return st.as_dict()

    def stream_count(self, region) -> int:
        """The allocated blocks `region` holds; nothing changes."""
        return self.stream_out_into(region, 0, None, None)[0]

    def stream_out(self, region, capacity: int = None, colors: bool = None) -> dict:
        """Takes the blocks of `region` out of the model and returns them in host memory: {"keys": int32 [n, 3], "voxels":
        [n, 512] {sdf, weight}, "colors": uint32 [n, 512] or None, "selected": the blocks the region held}.  n = min(selected,
        capacity); capacity=None counts first and takes them all.  colors=None: the colour travels if the table has any;
        colors=False drops it."""
        colors = self.has_color() if colors is None else bool(colors)
        cap = self.stream_count(region) if capacity is None else min(int(capacity), int(self.params.numVoxelBlocks))
        recs = np.zeros(cap, RECORD_DTYPE)
        cols = np.zeros((cap, 512), np.uint32) if colors else None
        sel, wr = C.c_uint64(), C.c_uint64()
        r = self._stream_region(region)
        L.check(self._lib.vh_stream_out_host(self._h, C.byref(r), cap, recs.ctypes.data_as(C.c_void_p) if cap else None,
                                             cols.ctypes.data_as(C.c_void_p) if colors and cap else None, C.byref(sel), C.byref(wr)),
                "vh_stream_out_host")
        n = int(wr.value)
        return {"keys": recs["pos"][:n].copy(), "voxels": recs["voxels"][:n].copy(), "colors": cols[:n].copy() if colors else None,
                "selected": int(sel.value)}

    def stream_in(self, chunk) -> dict:
        """Puts the blocks of `chunk` (what stream_out returns; "colors" may be None or missing) back into the model.  Returns
        vh_stream_stats as a dict plus "status": int32 [n], STREAM_PLACED / PRESENT / UNPLACED / FOREIGN per record."""
        keys = np.asarray(chunk["keys"], np.int32).reshape(-1, 3)
        n = len(keys)
        recs = np.zeros(n, RECORD_DTYPE)
        recs["pos"] = keys
        recs["voxels"] = np.asarray(chunk["voxels"], VOXEL_DTYPE).reshape(n, 512)
        cols = chunk.get("colors")
        if cols is not None:
            cols = np.ascontiguousarray(np.asarray(cols, np.uint32).reshape(n, 512))
        status = np.zeros(n, np.int32)
        st = L.StreamStats()
        L.check(self._lib.vh_stream_in_host(self._h, n, recs.ctypes.data_as(C.c_void_p) if n else None,
                                            cols.ctypes.data_as(C.c_void_p) if cols is not None and n else None,
                                            status.ctypes.data_as(C.c_void_p) if n else None, C.byref(st)), "vh_stream_in_host")
        out = st.as_dict()
        out["status"] = status
        return out

    # ---- the model as geometry (DESIGN.md "mesh") ----
    @staticmethod
    def _mesh_region(region):
        if region is None:
            return None
        lo, hi = region
        return C.byref(L.MeshRegion((C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi])))

    def extract_mesh_into(self, capacity: int, positions, normals=None, region=None) -> int:
        """vh_extract_mesh into caller-owned device buffers ([capacity, 3, 3] float32, or None with capacity 0);
        returns the triangles the region holds, which may exceed `capacity`."""
        n = C.c_uint64()
        L.check(self._lib.vh_extract_mesh(self._h, self._mesh_region(region), int(capacity), _dev_ptr(positions),
                                          _dev_ptr(normals), C.byref(n)), "vh_extract_mesh")
        return int(n.value)

    def mesh_count(self, region=None) -> int:
        """Triangles of the zero level inside `region` = ((lo x, y, z), (hi x, y, z)) in blocks, None = the whole model."""
        return self.extract_mesh_into(0, None, None, region)

    def extract_mesh(self, region=None, normals: bool = False, weld: bool = False):
        """The triangle mesh of the model (marching tetrahedra, world frame, wound towards free space), extracted on the GPU.
        weld=False: triangles [T, 3, 3] float32 (and per-vertex normals [T, 3, 3] with normals=True).
        weld=True: vertices [V, 3] float32 and faces [T, 3] int32 (shared vertices are bit-equal, so the welding is an exact
        `unique` on the host), and per-vertex normals [V, 3] with normals=True.  Returns a tuple in that order.
        The weld is by position bits, sorted on the host.  extract_mesh_indexed() gives the indexed form straight from the
        GPU, without the sort, and identifies a vertex by its cell edge: edges whose positions coincide (an sdf of +-0, keys
        beyond float32's integers) stay separate vertices there and are merged here, and the vertex order differs."""
        import torch
        count = self.mesh_count(region)
        with torch.cuda.device(self.device_index()):
            pos = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda")
            nrm = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda") if normals else None
        if count:
            got = self.extract_mesh_into(count, pos, nrm, region)
            if got != count:
                raise L.VoxelHashError(f"the model changed between the count ({count}) and the extraction ({got})")
        tris = pos.cpu().numpy()
        nn = nrm.cpu().numpy() if normals else None
        if not weld:
            return (tris, nn) if normals else tris
        from .mesh_io import weld_triangles
        verts, faces, first = weld_triangles(tris)
        return (verts, faces, nn.reshape(-1, 3)[first]) if normals else (verts, faces)

    def extract_mesh_indexed_into(self, capacity_vertices: int, capacity_triangles: int, vertices, indices, normals=None,
                                  region=None):
        """vh_extract_mesh_indexed into caller-owned device buffers (vertices, normals: [capacity_vertices, 3] float32;
        indices: [capacity_triangles, 3] int32 or uint32; None with a capacity of 0).  Returns (V, T), what the region holds,
        which may exceed the capacities."""
        nv, nt = C.c_uint64(), C.c_uint64()
        L.check(self._lib.vh_extract_mesh_indexed(self._h, self._mesh_region(region), int(capacity_vertices),
                                                  int(capacity_triangles), _dev_ptr(vertices), _dev_ptr(normals),
                                                  _dev_ptr(indices), C.byref(nv), C.byref(nt)), "vh_extract_mesh_indexed")
        return int(nv.value), int(nt.value)

    def mesh_counts(self, region=None):
        """(vertices, triangles) of the indexed mesh inside `region`, None = the whole model."""
        return self.extract_mesh_indexed_into(0, 0, None, None, None, region)

    def extract_mesh_indexed(self, region=None, normals: bool = False, colors: bool = False, labels: bool = False):
        """The mesh of extract_mesh() in indexed form, made on the GPU: (vertices [V, 3] float32, faces [T, 3] int32) and
        per-vertex normals [V, 3] with normals=True.  One vertex per cell edge with a sign change (never merged by position);
        vertices[faces] has the bits of extract_mesh(), triangle for triangle.  colors=True appends the per-vertex colour
        words [V] uint32 (r | g << 8 | b << 16 | 0xFF << 24; 0 = no colour; mesh_io.save_ply takes them as they are): the
        trilinear colour sample at the vertex where it has one, else the nearest voxel's.  labels=True appends (last) the
        per-vertex label words [V] uint32 (label | votes << 16; 0 = no label): the nearest voxel's, sample_labels()."""
        import torch
        nv, nt = self.mesh_counts(region)
        if nv > 2**31 - 1:
            raise L.VoxelHashError(f"{nv} vertices do not fit int32 faces: extract by regions")
        with torch.cuda.device(self.device_index()):
            pos = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
            idx = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
            nrm = torch.empty((nv, 3), dtype=torch.float32, device="cuda") if normals else None
        if nv or nt:
            got = self.extract_mesh_indexed_into(nv, nt, pos, idx, nrm, region)
            if got != (nv, nt):
                raise L.VoxelHashError(f"the model changed between the count ({nv}, {nt}) and the extraction {got}")
        out = (pos.cpu().numpy(), idx.cpu().numpy()) + ((nrm.cpu().numpy(),) if normals else ())
        if colors:
            tri = self.sample_color(pos, L.SAMPLE_TRILINEAR).cpu().numpy()
            near = self.sample_color(pos, L.SAMPLE_NEAREST).cpu().numpy()
            out += (np.where(tri != 0, tri, near),)
        if labels:
            out += (self.sample_labels(pos).cpu().numpy(),)
        return out

    # ---- incremental meshing ----
    _CHANGES_HALOS = {"none": L.CHANGES_HALO_NONE, "mesh": L.CHANGES_HALO_MESH, "normals": L.CHANGES_HALO_NORMALS}
    CHANGES_SLOT_DTYPE = np.dtype([("key", "<i4", (3,)), ("live", "<u4"), ("h0", "<u8"), ("h1", "<u8")])      # a slot of the state

    def changes_state_bytes(self) -> int:
        n = C.c_uint64()
        L.check(self._lib.vh_changes_state_bytes(self._h, C.byref(n)), "vh_changes_state_bytes")
        return int(n.value)

    def changes_state(self):
        """The empty state of vh_changes for this table: a zeroed CUDA tensor of uint8 (64 bytes of header, the first word the
        epoch, then 32 bytes per pool block).  The caller keeps it between calls of changes()."""
        import torch
        with torch.cuda.device(self.device_index()):
            return torch.zeros((self.changes_state_bytes(),), dtype=torch.uint8, device="cuda")

    def changes_into(self, state, capacity_changed: int, changed, capacity_removed: int, removed, region=None, color: bool = False,
                     halo="mesh"):
        """vh_changes into caller-owned device buffers: changed int32 [capacity_changed, 4] = {x, y, z, flags}, removed int32
        [capacity_removed, 4] (None with a capacity of 0).  Returns (changed, removed), the counts; the lists are written and
        `state` advances only if both fit, so capacities of 0 peek.  Synchronises."""
        what = L.CHANGES_VOXELS | (L.CHANGES_COLOR if color else 0)
        mode = self._CHANGES_HALOS[halo] if isinstance(halo, str) else int(halo)
        nc, nr = C.c_uint64(), C.c_uint64()
        L.check(self._lib.vh_changes(self._h, _dev_ptr(state), self._mesh_region(region), what, mode, int(capacity_changed),
                                     _dev_ptr(changed), int(capacity_removed), _dev_ptr(removed), C.byref(nc), C.byref(nr)),
                "vh_changes")
        return int(nc.value), int(nr.value)

    def changes(self, state, region=None, color: bool = False, halo="mesh"):
        """The blocks of `region` (None: the whole model) that differ from what `state` last saw, as CUDA tensors: (changed int32
        [n, 4] = {x, y, z, flags} in the table's entry order, flags CHANGED_SELF | CHANGED_HALO; removed int32 [m, 4]).  halo
        "mesh": also the blocks whose mesh reads a changed or removed block; "normals": ... whose mesh with normals does; "none".
        color=True: the colour words count as well.  The state advances.  The buffers are kept on the table and grown, and the
        call is made again, when a count does not fit: the tensors returned are views of them, valid until the next call."""
        import torch
        buf = getattr(self, "_changes_buffers", None)
        if buf is None:
            with torch.cuda.device(self.device_index()):
                buf = self._changes_buffers = [torch.empty((64, 4), dtype=torch.int32, device="cuda"),
                                               torch.empty((16, 4), dtype=torch.int32, device="cuda")]
        while True:
            nc, nr = self.changes_into(state, buf[0].shape[0], buf[0], buf[1].shape[0], buf[1], region, color, halo)
            if nc <= buf[0].shape[0] and nr <= buf[1].shape[0]:
                return buf[0][:nc], buf[1][:nr]
            with torch.cuda.device(self.device_index()):
                if nc > buf[0].shape[0]:
                    buf[0] = torch.empty((nc + nc // 2, 4), dtype=torch.int32, device="cuda")
                if nr > buf[1].shape[0]:
                    buf[1] = torch.empty((nr + nr // 2, 4), dtype=torch.int32, device="cuda")

    def extract_mesh_blocks_into(self, keys, capacity: int, positions, normals=None, first=None, n: int = None) -> int:
        """vh_extract_mesh_blocks into caller-owned device buffers: keys int32 [n, 4] (the 4th word is ignored), positions and
        normals [capacity, 3, 3] float32 (None with capacity 0), first [n + 1] int64 / uint64 or None.  Returns the triangles
        the keys' blocks hold, which may exceed `capacity`."""
        n = int(keys.shape[0]) if n is None else int(n)
        t = C.c_uint64()
        L.check(self._lib.vh_extract_mesh_blocks(self._h, n, _dev_ptr(keys) if n else None, int(capacity), _dev_ptr(positions),
                                                 _dev_ptr(normals), _dev_ptr(first), C.byref(t)), "vh_extract_mesh_blocks")
        return int(t.value)

    def extract_mesh_blocks(self, keys, normals: bool = False):
        """The triangles of the blocks `keys` (int32 [n, 3 or 4], a CUDA tensor or anything numpy takes; changes()'s first result
        as it is), block by block: (positions [T, 3, 3] float32, normals [T, 3, 3] or None, first uint64 [n + 1]) in host
        memory.  Block j's triangles are positions[first[j]:first[j + 1]], the bytes of extract_mesh(region=(j, j + 1)); an
        absent key has none."""
        import torch
        with torch.cuda.device(self.device_index()):
            if not isinstance(keys, torch.Tensor):
                k = np.asarray(keys, np.int32)
                k = k.reshape(-1, k.shape[-1] if k.ndim > 1 else 3)
                keys = torch.from_numpy(np.ascontiguousarray(k)).cuda()
            if keys.shape[-1] == 3:
                keys = torch.cat([keys, torch.zeros_like(keys[:, :1])], dim=1)
            keys = keys.to(torch.int32).contiguous()
            n = int(keys.shape[0])
            first = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
            count = self.extract_mesh_blocks_into(keys, 0, None, None, first) if n else 0
            pos = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda")
            nrm = torch.empty((count, 3, 3), dtype=torch.float32, device="cuda") if normals else None
        if count:
            got = self.extract_mesh_blocks_into(keys, count, pos, nrm, first)
            if got != count:
                raise L.VoxelHashError(f"the model changed between the count ({count}) and the extraction ({got})")
        return pos.cpu().numpy(), (nrm.cpu().numpy() if normals else None), first.cpu().numpy().view(np.uint64)

    # ---- the model as a distance field ----
    def sample_sdf_into(self, points, sdf, weight=None, gradient=None, mode: int = L.SAMPLE_TRILINEAR, n: int = None):
        """vh_sample_sdf into caller-owned device buffers: points [n, 3] float32 (world metres), sdf [n], weight [n] or None,
        gradient [n, 3] or None.  Asynchronous on the context's stream."""
        n = int(points.shape[0]) if n is None else int(n)
        L.check(self._lib.vh_sample_sdf(self._h, int(mode), n, _dev_ptr(points), _dev_ptr(sdf), _dev_ptr(weight),
                                        _dev_ptr(gradient)), "vh_sample_sdf")
        return sdf

    def sample_sdf(self, points, mode: int = L.SAMPLE_TRILINEAR, weight: bool = False, gradient: bool = False):
        """The TSDF at world points [n, 3] (float32 CUDA tensor): sdf [n] (NaN where there is no valid sample), then
        weight [n] and gradient [n, 3] (per world metre) when asked for, as CUDA tensors; a tuple when more than one."""
        import torch
        n = int(points.shape[0])
        sdf = torch.empty((n,), dtype=torch.float32, device=points.device)
        w = torch.empty((n,), dtype=torch.float32, device=points.device) if weight else None
        g = torch.empty((n, 3), dtype=torch.float32, device=points.device) if gradient else None
        self.sample_sdf_into(points, sdf, w, g, mode)
        out = (sdf,) + ((w,) if weight else ()) + ((g,) if gradient else ())
        return out if len(out) > 1 else sdf

    def sample_lattice_into(self, lo, dims, sdf, weight=None):
        """vh_sample_lattice into caller-owned device buffers of dims[0] * dims[1] * dims[2] floats, x fastest."""
        lo3, d3 = (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in dims])
        L.check(self._lib.vh_sample_lattice(self._h, lo3, d3, _dev_ptr(sdf), _dev_ptr(weight)), "vh_sample_lattice")
        return sdf

    def sample_lattice(self, lo, dims, weight: bool = False):
        """The voxels lo <= g < lo + dims (global voxel coordinates, x, y, z) as a CUDA tensor [dims[2], dims[1], dims[0]]:
        the stored sdf, NaN where the voxel is not valid; with weight=True also the weights (0 where not valid)."""
        import torch
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        with torch.cuda.device(self.device_index()):
            sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
            w = torch.empty(shape, dtype=torch.float32, device="cuda") if weight else None
        self.sample_lattice_into(lo, dims, sdf, w)
        return (sdf, w) if weight else sdf

    # ---- the Euclidean distance to the surface ----
    def esdf_workspace_bytes(self, dims, radius: int) -> int:
        """Bytes of workspace vh_esdf_lattice needs for a box of `dims` at `radius` (0 for an empty box)."""
        d3, n = (C.c_int32 * 3)(*[int(v) for v in dims]), C.c_uint64(0)
        L.check(self._lib.vh_esdf_workspace_bytes(d3, int(radius), C.byref(n)), "vh_esdf_workspace_bytes")
        return int(n.value)

    def esdf_lattice_into(self, lo, dims, radius: int, dist2, distance=None, unknown: int = L.ESDF_UNKNOWN_KEEP, workspace=None):
        """vh_esdf_lattice into caller-owned device buffers of dims[0] * dims[1] * dims[2] elements, x fastest: dist2 (int32) or
        None, distance (float32, metres) or None; workspace: a CUDA byte tensor of at least esdf_workspace_bytes(dims, radius)
        bytes, 16-byte aligned (None: a torch byte tensor is allocated for this call and given back to torch's allocator once
        the context's stream has passed the launches that use it: nothing is kept between calls, so a loop over many boxes
        does better with a workspace of its own).  Asynchronous on the context's stream."""
        lo3, d3 = (C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in dims])
        own = workspace is None
        if own:
            import torch
            with torch.cuda.device(self.device_index()):
                workspace = torch.empty((max(self.esdf_workspace_bytes(dims, radius), 16),), dtype=torch.uint8, device="cuda")
        L.check(self._lib.vh_esdf_lattice(self._h, lo3, d3, int(radius), int(unknown), _dev_ptr(workspace),
                                          int(workspace.numel() * workspace.element_size()), _dev_ptr(dist2), _dev_ptr(distance)),
                "vh_esdf_lattice")
        if own:                                     # the launches are only queued: no reuse before the context's stream is past them
            dev = self.device_index()
            workspace.record_stream(torch.cuda.ExternalStream(self.stream_handle, device=dev) if self.stream_handle
                                    else torch.cuda.default_stream(dev))
        return dist2 if dist2 is not None else distance

    def esdf_lattice(self, lo, dims, radius: int, unknown: int = L.ESDF_UNKNOWN_KEEP, distance: bool = True, dist2: bool = False):
        """The Euclidean signed distance to the surface at the voxels lo <= g < lo + dims, up to `radius` voxels, as CUDA tensors
        [dims[2], dims[1], dims[0]]: the distance in metres (float32; +-inf: nothing of the other class within the radius, NaN:
        an unknown voxel) and / or the exact signed squared distance in voxels (int32; ESDF_FAR, ESDF_NONE); a tuple
        (distance, dist2) when both are asked for."""
        import torch
        if not (distance or dist2):
            raise ValueError("ask for distance, dist2 or both")
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        with torch.cuda.device(self.device_index()):
            f = torch.empty(shape, dtype=torch.float32, device="cuda") if distance else None
            d = torch.empty(shape, dtype=torch.int32, device="cuda") if dist2 else None
        self.esdf_lattice_into(lo, dims, radius, d, f, unknown)
        return (f, d) if distance and dist2 else f if distance else d

    # ---- connected pieces of the model ----
    COMPONENT_DTYPE = np.dtype([("voxel", "<i4", (3,)), ("size", "<u4")])          # vh_component
    _COMPONENT_TARGETS = {"inside": L.COMPONENT_INSIDE, "outside": L.COMPONENT_OUTSIDE}

    def _component_target(self, target):
        return self._COMPONENT_TARGETS[target] if isinstance(target, str) else int(target)

    def components_into(self, capacity: int, records, lo=None, dims=None, labels=None, region=None, target="inside",
                        connectivity: int = 14) -> dict:
        """vh_components into caller-owned device buffers: records [capacity] of COMPONENT_DTYPE's 16 bytes (None with capacity
        0), labels dims[0] * dims[1] * dims[2] uint32 (or int32) over the box lo, dims, x fastest (all three None: no labels).
        Returns the stats as a dict; `components` may exceed `capacity`.  Synchronises."""
        lo3 = (C.c_int32 * 3)(*[int(v) for v in lo]) if lo is not None else None
        d3 = (C.c_int32 * 3)(*[int(v) for v in dims]) if dims is not None else None
        st = L.ComponentStats()
        L.check(self._lib.vh_components(self._h, self._mesh_region(region), self._component_target(target), int(connectivity),
                                        int(capacity), _dev_ptr(records), lo3, d3, _dev_ptr(labels), C.byref(st)), "vh_components")
        return st.as_dict()

    def components(self, region=None, target="inside", connectivity: int = 14, lattice=None):
        """The connected pieces of the model: (records, labels, stats).  target "inside": the valid voxels with sdf <= 0, what the
        mesh shows as closed pieces; "outside": the other valid voxels.  connectivity 6 or 14 (the mesh's own tetrahedra).
        records: a numpy array of COMPONENT_DTYPE (global voxel of the root, size) in output order; labels: with lattice =
        (lo, dims) a CUDA tensor [dims[2], dims[1], dims[0]] int32 holding each voxel's index into records, -1 (the bits of
        COMPONENT_NONE) where the voxel is no node; else None; stats: a dict of vh_component_stats."""
        import torch
        count = self.components_into(0, None, region=region, target=target, connectivity=connectivity)["components"]
        lo, dims = lattice if lattice is not None else (None, None)
        with torch.cuda.device(self.device_index()):
            rec = torch.empty((max(count, 1), 4), dtype=torch.int32, device="cuda")
            lab = torch.empty((int(dims[2]), int(dims[1]), int(dims[0])), dtype=torch.int32, device="cuda") if lattice is not None else None
        stats = self.components_into(count, rec if count else None, lo, dims, lab, region, target, connectivity)
        if stats["components"] != count:
            raise L.VoxelHashError(f"the model changed between the count ({count}) and the labelling ({stats['components']})")
        records = rec[:count].cpu().numpy().view(self.COMPONENT_DTYPE).reshape(count)
        return records, lab, stats

    def remove_components(self, min_size: int, region=None, target="inside", connectivity: int = 14) -> dict:
        """vh_remove_components: every component with fewer than `min_size` nodes is cleared out of the volume (voxels {0, 0},
        colour 0), and the blocks that emptied are freed.  Returns the stats as a dict.  Synchronises."""
        st = L.ComponentStats()
        L.check(self._lib.vh_remove_components(self._h, self._mesh_region(region), self._component_target(target),
                                               int(connectivity), int(min_size), C.byref(st)), "vh_remove_components")
        return st.as_dict()

    # ---- the model met by rays ----
    def cast_rays_into(self, rays, t, normals=None, voxels=None, depth_plane=None, n: int = None):
        """vh_cast_rays into caller-owned device buffers: rays [n, 8] float32 (origin, t_min, direction, t_max; 16-byte
        aligned), t [n], normals [n, 3] float32 or None, voxels [n, 4] int32 or None; depth_plane: four host floats (one
        plane places the samples of all rays: row 2 of a pose's inverse gives vh_raycast's depths) or None (along each ray).
        Asynchronous on the context's stream."""
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError("rays must be a float32 tensor [n, 8]")
        n = int(rays.shape[0]) if n is None else int(n)
        if not 0 <= n <= rays.shape[0]:
            raise ValueError(f"n = {n} but rays holds {rays.shape[0]}")
        for name, buf, dtype, per in (("t", t, torch.float32, 1), ("normals", normals, torch.float32, 3),
                                      ("voxels", voxels, torch.int32, 4)):
            if buf is None and name != "t":
                continue
            if buf is None or buf.dtype != dtype or buf.numel() < per * n:
                raise ValueError(f"{name} must be a {dtype} tensor of at least {per} * n = {per * n} elements")
        plane = None
        if depth_plane is not None:
            p = np.ascontiguousarray(np.asarray(depth_plane, np.float32).reshape(4))
            plane = p.ctypes.data_as(C.POINTER(C.c_float))
        L.check(self._lib.vh_cast_rays(self._h, n, _dev_ptr(rays), plane, _dev_ptr(t), _dev_ptr(normals), _dev_ptr(voxels)),
                "vh_cast_rays")
        return t

    def cast_rays(self, rays, depth_plane=None, normals: bool = False, voxels: bool = False):
        """Where the rays [n, 8] (float32 CUDA tensor: origin, t_min, direction, t_max) meet the surface: t [n] (NaN where
        they do not), then the world-frame normals [n, 3] and the hit voxels with the status word [n, 4] (int32; 1 hit, 0 miss,
        -1 refused) when asked for, as CUDA tensors; a tuple when more than one."""
        import torch
        n = int(rays.shape[0])
        t = torch.empty((n,), dtype=torch.float32, device=rays.device)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=rays.device) if normals else None
        vox = torch.empty((n, 4), dtype=torch.int32, device=rays.device) if voxels else None
        self.cast_rays_into(rays, t, nrm, vox, depth_plane)
        out = (t,) + ((nrm,) if normals else ()) + ((vox,) if voxels else ())
        return out if len(out) > 1 else t

    def device_index(self) -> int:
        """Ordinal of the device the context lives on."""
        import torch
        dev = getattr(self, "_device", -1)
        return torch.cuda.current_device() if dev is None or dev < 0 else dev

    # ---- raycast over shards (DESIGN.md section 6 "raycast") ----
    VIEW_RECORD_BYTES = 4112

    def export_views(self, poses, records, capacity: int, counts, t_min: float = 0.1, t_max: float = 5.0):
        """poses: [n][16] host; records: device uint8 [n*capacity, 4112]; counts: device int32 [n]."""
        p = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16))
        L.check(self._lib.vh_export_views(self._h, p.ctypes.data_as(C.POINTER(C.c_float)), p.shape[0], t_min, t_max,
                                          _dev_ptr(records), capacity, _dev_ptr(counts)), "vh_export_views")

    def export_views_fixed(self, d_poses, n_views: int, records, capacity: int, counts, t_min: float = 0.1,
                           t_max: float = 5.0):
        """The same with device poses [n_views, 16] and fixed slots: view v's records at records[v*capacity:]."""
        L.check(self._lib.vh_export_views_fixed(self._h, _dev_ptr(d_poses), int(n_views), t_min, t_max, _dev_ptr(records),
                                                capacity, _dev_ptr(counts)), "vh_export_views_fixed")

    def import_views(self, records, num_sources: int, capacity: int, counts):
        """Fixed-slot import: source s holds min(counts[s], capacity) records at records[s*capacity:] (counts on the device)."""
        self._view_records = records
        L.check(self._lib.vh_import_views(self._h, _dev_ptr(records), int(num_sources), int(capacity), _dev_ptr(counts)),
                "vh_import_views")

    def import_view(self, records, count: int):
        """Make this dedicated, unsharded context hold exactly records[:count] (voxels stay in `records`)."""
        self._view_records = records            # keep the buffer alive while the table points into it
        L.check(self._lib.vh_import_view(self._h, _dev_ptr(records), int(count)), "vh_import_view")

    # ---- step-level entry points (VoxelUtils.h:5-13) ----
    def set_pose(self, pose):
        _, pp = _pose16(pose)
        L.check(self._lib.vh_set_pose(self._h, pp), "vh_set_pose")

    def reset_mutexes(self):
        L.check(self._lib.vh_reset_mutexes(self._h), "vh_reset_mutexes")

    def alloc_blocks(self, verts, normals=None):
        L.check(self._lib.vh_alloc_blocks(self._h, _dev_ptr(verts), _dev_ptr(normals)), "vh_alloc_blocks")

    def flatten(self, sync: bool = True):
        if not sync:
            L.check(self._lib.vh_flatten(self._h, None), "vh_flatten")
            return None
        n = C.c_int32()
        L.check(self._lib.vh_flatten(self._h, C.byref(n)), "vh_flatten")
        return n.value

    def integrate_depth_map(self, verts):
        L.check(self._lib.vh_integrate_depth_map(self._h, _dev_ptr(verts)), "vh_integrate_depth_map")

    # ---- sharding ----
    def generate_keys(self, verts, camera_id: int, num_shards: int, bins_out, capacity: int, packet_out=None,
                      bin_stride: int = 0):
        """Key bins (capacity records each, `bin_stride` records apart) + the camera packet for the
        pose set with set_pose().  bins_out / packet_out: device tensors or raw addresses."""
        L.check(self._lib.vh_generate_keys(self._h, _dev_ptr(verts), camera_id, num_shards, _dev_ptr(bins_out),
                                           capacity, bin_stride, _dev_ptr(packet_out)), "vh_generate_keys")

    def insert_bins(self, bins, num_bins: int, capacity: int, bin_stride: int = 0):
        L.check(self._lib.vh_insert_bins(self._h, _dev_ptr(bins), num_bins, capacity, bin_stride), "vh_insert_bins")

    def integrate_packets(self, num_cams: int, packets, packet_stride: int = 0):
        L.check(self._lib.vh_integrate_packets(self._h, num_cams, _dev_ptr(packets), packet_stride),
                "vh_integrate_packets")

    def generate_keys_batch(self, poses16, vert_ptrs, camera_id: int, num_shards: int, bins_out, capacity: int,
                            packets_out, batch: int, per_batch_bins: bool = False):
        """`batch` frames of this camera in one call.  poses16: float32 [batch, 16] (contiguous numpy),
        vert_ptrs: ctypes array of `batch` device addresses; bins_out [num_shards, batch, capacity, 4],
        packets_out [batch, 32 + W*H] (dense layouts).  per_batch_bins: bins_out [num_shards, capacity, 4], one bin per
        shard for the whole batch (VH_BIN_PER_BATCH)."""
        L.check(self._lib.vh_generate_keys_batch(
            self._h, batch, poses16.ctypes.data_as(C.POINTER(C.c_float)), vert_ptrs, camera_id, num_shards,
            _dev_ptr(bins_out), capacity, 0, -1 if per_batch_bins else 0, _dev_ptr(packets_out), 0), "vh_generate_keys_batch")

    def generate_keys_depth_batch(self, poses16, depth_ptrs, k_inv, camera_id: int, num_shards: int, bins_out,
                                  capacity: int, packets_out, batch: int, per_batch_bins: bool = False):
        """Keys + sensor-depth packets of `batch` frames from the uint16 images alone (dense layouts)."""
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_generate_keys_depth_batch(
            self._h, batch, poses16.ctypes.data_as(C.POINTER(C.c_float)), depth_ptrs,
            k.ctypes.data_as(C.POINTER(C.c_float)), camera_id, num_shards, _dev_ptr(bins_out), capacity, 0,
            -1 if per_batch_bins else 0, _dev_ptr(packets_out), 0), "vh_generate_keys_depth_batch")

    def write_packets_u16_batch(self, poses16, depth_ptrs, k_inv, packets_out, batch: int, packet_frame_stride: int = 0):
        """Sensor-depth packets (VH_PACKET_U16) of `batch` frames: depth_ptrs = ctypes array of device
        addresses of W*H uint16 images; packets_out: device tensor or address, [batch, 36 + W*H/2] floats."""
        k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        L.check(self._lib.vh_write_packets_u16_batch(
            self._h, batch, poses16.ctypes.data_as(C.POINTER(C.c_float)), depth_ptrs,
            k.ctypes.data_as(C.POINTER(C.c_float)), _dev_ptr(packets_out), packet_frame_stride),
            "vh_write_packets_u16_batch")

    def apply_frames_batch(self, bins, num_bins: int, capacity: int, num_cams: int, packets, batch: int,
                           per_batch_bins: bool = False):
        """Apply `batch` multi-camera frames: bins [num_bins, batch, capacity, 4] (per_batch_bins: [num_bins, capacity, 4]),
        packets [num_cams, batch, 32 + W*H] (dense layouts)."""
        L.check(self._lib.vh_apply_frames_batch(self._h, batch, _dev_ptr(bins), num_bins, capacity, 0,
                                                -1 if per_batch_bins else 0, num_cams, _dev_ptr(packets), 0, 0),
                "vh_apply_frames_batch")

    # ---- model dump / checkpoint ----
    def dump_sdf_text(self, path: str):
        """SDF_dump.txt in the format of SDFRenderer::printSDFdata (SDFRenderer.cpp:71-110)."""
        L.check(self._lib.vh_dump_sdf_text(self._h, str(path).encode()), "vh_dump_sdf_text")

    def save_snapshot(self, path: str):
        L.check(self._lib.vh_save_snapshot(self._h, str(path).encode()), "vh_save_snapshot")

    def load_snapshot(self, path: str):
        L.check(self._lib.vh_load_snapshot(self._h, str(path).encode()), "vh_load_snapshot")

    # ---- queries ----
    def synchronize(self):
        L.check(self._lib.vh_synchronize(self._h), "vh_synchronize")

    def counters(self) -> dict:
        c = L.Counters()
        L.check(self._lib.vh_get_counters(self._h, C.byref(c)), "vh_get_counters")
        return c.as_dict()

    def device_pointers(self) -> L.PtrContainer:
        p = L.PtrContainer()
        L.check(self._lib.vh_get_device_pointers(self._h, C.byref(p)), "vh_get_device_pointers")
        return p

    @property
    def num_entries(self) -> int:
        lo, hi = self.bucket_range
        return (hi - lo) * self.params.bucketSize

    def _download(self, which, dtype, count):
        out = np.empty(count, dtype)
        if count:
            L.check(self._lib.vh_download(self._h, which, out.ctypes.data_as(C.c_void_p), out.nbytes), "vh_download")
        return out

    def hash_table(self) -> np.ndarray:
        return self._download(L.BUF_HASH_TABLE, ENTRY_DTYPE, self.num_entries)

    def compact(self) -> np.ndarray:
        n = self.counters()["occupied"]
        return self._download(L.BUF_COMPACT, ENTRY_DTYPE, n)

    def sdf_blocks(self) -> np.ndarray:
        return self._download(L.BUF_SDF_BLOCKS, VOXEL_DTYPE, self.params.numVoxelBlocks * 512)

    def heap(self) -> np.ndarray:
        return self._download(L.BUF_HEAP, np.dtype("<u4"), self.params.numVoxelBlocks)

    def block_voxels(self, ptr: int) -> np.ndarray:
        """The 512 voxels of the block at voxel index `ptr` (an entry's ptr), without the rest of the volume."""
        out = np.empty(512, VOXEL_DTYPE)
        L.check(self._lib.vh_download_range(self._h, L.BUF_SDF_BLOCKS, 8 * int(ptr), out.ctypes.data_as(C.c_void_p),
                                            out.nbytes), "vh_download_range")
        return out

    def allocated(self) -> np.ndarray:
        t = self.hash_table()
        return t[t["ptr"] != L.FREE_BLOCK]

    def debug_eval(self, points, out):
        L.check(self._lib.vh_debug_eval(self._h, _dev_ptr(points), points.shape[0], _dev_ptr(out)), "vh_debug_eval")

    def set_option(self, name: str, value: int):
        L.check(self._lib.vh_set_option(self._h, name.encode(), int(value)), "vh_set_option")

    def set_profiling(self, on: bool):
        L.check(self._lib.vh_set_profiling(self._h, int(on)), "vh_set_profiling")

    def kernel_times(self, reset: bool = True) -> dict:
        t = L.KernelTimes()
        L.check(self._lib.vh_get_kernel_times(self._h, C.byref(t), int(reset)), "vh_get_kernel_times")
        return t.as_dict()
