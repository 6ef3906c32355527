"""Host-side mirror of the reference's CameraTracking (CameraTracking.h:36-59) for Python callers:
frame-to-frame point-to-plane ICP on the GPU through the C-ABI (vh_icp_*), plus the helpers that
turn a raycast of the model into an ICP target (frame-to-model tracking).  No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

ICP_ABS_DISTANCE, ICP_NEED_TARGET = 1, 2
DIST_THRES = 0.08          # common.h:12
MAX_ITERS = 20             # CameraTracking.h:40


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def se3_exp(twist) -> np.ndarray:
    t, T = np.ascontiguousarray(twist, np.float64), np.zeros(16)
    L.load().vh_se3_exp(_dp(t), _dp(T))
    return T.reshape(4, 4)


def se3_log(T) -> np.ndarray:
    T, t = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16)), np.zeros(6)
    L.load().vh_se3_log(_dp(T), _dp(t))
    return t


def system_arrays(sys: L.IcpSystem):
    return (np.array(sys.JTJ, np.float64).reshape(6, 6), np.array(sys.JTr, np.float64), float(sys.error),
            int(sys.count))


def icp_solve(JTJ, JTr, estimate):
    """-> (ok, new estimate): update = -(JTJ^-1 JTr), estimate = log(exp(update) exp(estimate))."""
    sys = L.IcpSystem()
    sys.JTJ[:] = np.asarray(JTJ, np.float64).reshape(36).tolist()
    sys.JTr[:] = np.asarray(JTr, np.float64).reshape(6).tolist()
    est = np.ascontiguousarray(estimate, np.float64).copy()
    rc = L.load().vh_icp_solve(C.byref(sys), _dp(est))
    return rc == 0, est


def depth_to_maps(depth, k_inv, positions, normals, stream=None):
    """float depth [H, W] in metres on the device -> float4 vertex and normal maps (in place)."""
    H, W = depth.shape
    k = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
    handle = 0 if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
    L.check(L.load().vh_depth_to_maps(_ptr(depth), _fp(k), W, H, _ptr(positions), _ptr(normals), C.c_void_p(handle)),
            "vh_depth_to_maps")
    return positions, normals


class CameraTracking:
    """CameraTracking(width, height); Align(input, target, target_normals) -> getTransform()."""

    def __init__(self, width: int, height: int, K, device: int = -1, stream=None, dist_thres: float = DIST_THRES,
                 max_iters: int = MAX_ITERS, flags: int = 0):
        self._lib = L.load()
        self.width, self.height = width, height
        self.K = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        self.dist_thres, self.max_iters, self.flags = dist_thres, max_iters, flags
        h = C.c_void_p()
        L.check(self._lib.vh_icp_create(width, height, device, C.byref(h)), "vh_icp_create")
        self._h = h
        if stream is not None:
            L.check(self._lib.vh_icp_set_stream(self._h, C.c_void_p(stream if isinstance(stream, int)
                                                                      else stream.cuda_stream)), "vh_icp_set_stream")
        self.delta = np.eye(4, dtype=np.float32)
        self.last = None
        self.iterations = 0

    def close(self):
        if self._h:
            self._lib.vh_icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_system(self, inp, target, target_normals, delta):
        d = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_icp_build_system(self._h, _ptr(inp), _ptr(target), _ptr(target_normals), _fp(d),
                                              _fp(self.K), self.dist_thres, self.flags, C.byref(sys)),
                "vh_icp_build_system")
        return system_arrays(sys)

    def correspondences(self, inp, target, target_normals, delta, corres, corres_normals, residuals):
        d = np.ascontiguousarray(np.asarray(delta, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_icp_correspondences(self._h, _ptr(inp), _ptr(target), _ptr(target_normals), _fp(d),
                                                 _fp(self.K), self.dist_thres, self.flags, _ptr(corres),
                                                 _ptr(corres_normals), _ptr(residuals), C.byref(sys)),
                "vh_icp_correspondences")
        return system_arrays(sys)

    def Align(self, inp, target, target_normals, start=None):
        """CameraTracking::Align: up to max_iters rounds; the result is kept in `delta` (getTransform)."""
        d = np.ascontiguousarray(np.asarray(np.eye(4) if start is None else start, np.float32).reshape(16)).copy()
        sys, it = L.IcpSystem(), C.c_int32()
        L.check(self._lib.vh_icp_align(self._h, _ptr(inp), _ptr(target), _ptr(target_normals), _fp(self.K),
                                       self.dist_thres, self.max_iters, self.flags, _fp(d), C.byref(sys),
                                       C.byref(it)), "vh_icp_align")
        self.delta, self.last, self.iterations = d.reshape(4, 4), system_arrays(sys), int(it.value)
        return self.delta

    def getTransform(self) -> np.ndarray:
        return self.delta


class FusionLoop:
    """The demo's frame order as a closed loop (Application.cpp:73-90: preProcess -> Align -> integrate, then the
    renderer reads the model; CameraTracking.cpp:26-69): per uint16 sensor frame

        vh_preprocess(depth)            -> input vertex map             (CameraTrackingUtils.cu:115-120)
        vh_icp_align(input, model maps) -> delta, pose = pose . delta   (frame-to-model: the target is the raycast)
        vh_integrate_depth(pose, depth) -> the model takes the frame    (SDF_Hashtable.cpp:11-40)
        vh_raycast_maps(pose)           -> depth + vertex + normal maps of the model for the next frame's Align

    all queued on ONE stream (the table's; the tracker is bound to it).  The only host synchronisation of a frame is the
    one inside vh_icp_align, which hands the 4x4 delta to the host -- the pose is a host value in the reference's
    interface (integrate(const float4x4&, ...)), so the next frame's calls cannot be queued before it is known.
    The first frame is integrated at `start_pose`."""

    def __init__(self, table, K, k_inv, stream=None, flags: int = ICP_ABS_DISTANCE | ICP_NEED_TARGET, max_iters: int = MAX_ITERS):
        import torch
        self.table, self.W, self.H = table, table.width, table.height
        self.k_inv = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        self.trk = CameraTracking(self.W, self.H, K, stream=stream, flags=flags, max_iters=max_iters)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.depth = torch.zeros((self.H, self.W), dtype=torch.float32, device=dev)
        self.model_v, self.model_n, self.in_v, self.in_n = (torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev)
                                                            for _ in range(4))
        self.stream = stream
        self.pose = None
        self.frames = 0

    def start(self, depth_u16, start_pose):
        self.pose = np.asarray(start_pose, np.float64).reshape(4, 4).copy()
        self.table.integrate_depth(self.pose.astype(np.float32), depth_u16, self.k_inv)
        self.table.raycast_maps(self.pose.astype(np.float32), self.depth, self.model_v, self.model_n)
        self.frames = 1
        return self.pose

    def track(self, depth_u16):
        """pre-process + Align only: the new pose (not yet integrated)."""
        from .hashtable import preprocess
        preprocess(depth_u16, self.k_inv, self.in_v, self.in_n, stream=self.stream)
        delta = self.trk.Align(self.in_v, self.model_v, self.model_n).astype(np.float64)
        self.pose = self.pose @ delta
        return self.pose

    def fuse(self, depth_u16):
        """integrate at the current pose + the model's maps for the next Align."""
        p32 = self.pose.astype(np.float32)
        self.table.integrate_depth(p32, depth_u16, self.k_inv)
        self.table.raycast_maps(p32, self.depth, self.model_v, self.model_n)
        self.frames += 1

    def step(self, depth_u16):
        """track + fuse in one library call (vh_fusion_step): the frame's five stages and the pose update without a return to
        Python in between."""
        sys, it = L.IcpSystem(), C.c_int32()
        trk = self.trk
        pose = np.ascontiguousarray(self.pose, np.float64)
        L.check(trk._lib.vh_fusion_step(self.table._h, trk._h, _ptr(depth_u16), _fp(self.k_inv), _fp(trk.K), trk.dist_thres,
                                        trk.max_iters, trk.flags, 0.1, 5.0, _ptr(self.in_v), _ptr(self.in_n), _ptr(self.depth),
                                        _ptr(self.model_v), _ptr(self.model_n), pose.ctypes.data_as(C.POINTER(C.c_double)),
                                        C.byref(sys), C.byref(it)), "vh_fusion_step")
        self.pose = pose
        trk.last, trk.iterations = system_arrays(sys), int(it.value)
        self.frames += 1
        return self.pose

    def close(self):
        self.trk.close()


SDF_MAX_ITERS = 10


class SdfTracking:
    """Point-to-SDF alignment against the table's own distance field (vh_sdf_*: no raycast, no projective pairing).
    SdfTracking(table); Align(input, start_pose) -> the camera -> world pose.  `K` is not needed by the rule and only kept.
    For models fused with a truncation of a few voxels (include/voxelhash.h, "tracking against the model itself")."""

    def __init__(self, table, K=None, dist_thres: float = DIST_THRES, max_iters: int = SDF_MAX_ITERS, width=None, height=None,
                 stream=None):
        self._lib = L.load()
        self.table = table
        self.width, self.height = width or table.width, height or table.height
        self.K = None if K is None else np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        self.dist_thres, self.max_iters = dist_thres, max_iters
        h = C.c_void_p()
        L.check(self._lib.vh_icp_create(self.width, self.height, -1, C.byref(h)), "vh_icp_create")
        self._h = h
        # the workspace must be bound to the table's stream: the table's own unless the caller names one
        self.stream_handle = table.stream_handle if stream is None else (stream if isinstance(stream, int) else stream.cuda_stream)
        L.check(self._lib.vh_icp_set_stream(self._h, C.c_void_p(self.stream_handle)), "vh_icp_set_stream")
        self.pose = np.eye(4)
        self.last = None
        self.iterations = 0

    def close(self):
        if self._h:
            self._lib.vh_icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_system(self, inp, pose):
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_sdf_build_system(self.table._h, self._h, _ptr(inp), _fp(p), self.dist_thres, C.byref(sys)),
                "vh_sdf_build_system")
        return system_arrays(sys)

    def residuals(self, inp, pose, points, sdf, gradient):
        """The system, and per pixel the moved point [H, W, 3], the residual [H, W] and the gradient [H, W, 3] (in place)."""
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_sdf_residuals(self.table._h, self._h, _ptr(inp), _fp(p), self.dist_thres, _ptr(points), _ptr(sdf),
                                           _ptr(gradient), C.byref(sys)), "vh_sdf_residuals")
        return system_arrays(sys)

    def Align(self, inp, start_pose):
        """Up to max_iters rounds from `start_pose` (e.g. the pose of the frame before); the result is kept in `pose`."""
        p = np.ascontiguousarray(np.asarray(start_pose, np.float64).reshape(16)).copy()
        sys, it = L.IcpSystem(), C.c_int32()
        L.check(self._lib.vh_sdf_align(self.table._h, self._h, _ptr(inp), self.dist_thres, self.max_iters, _dp(p), C.byref(sys),
                                       C.byref(it)), "vh_sdf_align")
        self.pose, self.last, self.iterations = p.reshape(4, 4), system_arrays(sys), int(it.value)
        return self.pose


class SdfFusionLoop:
    """The closed loop without a raycast: per uint16 sensor frame

        vh_preprocess(depth)              -> input vertex map
        vh_sdf_align(input, start = pose) -> pose          (against the model as fused so far)
        vh_integrate_depth(pose, depth)   -> the model takes the frame

    all on the table's stream; the one host synchronisation of a frame is vh_sdf_align's.  The first frame is integrated at
    `start_pose`."""

    def __init__(self, table, k_inv, K=None, stream=None, dist_thres: float = DIST_THRES, max_iters: int = SDF_MAX_ITERS):
        import torch
        self.table, self.W, self.H = table, table.width, table.height
        self.k_inv = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        self.trk = SdfTracking(table, K, dist_thres=dist_thres, max_iters=max_iters, stream=stream)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.in_v, self.in_n = (torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev) for _ in range(2))
        self.stream = self.trk.stream_handle
        self.pose = None
        self.frames = 0

    def start(self, depth_u16, start_pose):
        self.pose = np.asarray(start_pose, np.float64).reshape(4, 4).copy()
        self.table.integrate_depth(self.pose.astype(np.float32), depth_u16, self.k_inv)
        self.frames = 1
        return self.pose

    def track(self, depth_u16):
        """pre-process + Align only: the new pose (not yet integrated)."""
        from .hashtable import preprocess
        preprocess(depth_u16, self.k_inv, self.in_v, self.in_n, stream=self.stream)
        self.pose = self.trk.Align(self.in_v, self.pose)
        return self.pose

    def fuse(self, depth_u16):
        """integrate at the current pose."""
        self.table.integrate_depth(self.pose.astype(np.float32), depth_u16, self.k_inv)
        self.frames += 1

    def step(self, depth_u16):
        """track + fuse in one library call (vh_fusion_step_sdf)."""
        sys, it = L.IcpSystem(), C.c_int32()
        trk = self.trk
        pose = np.ascontiguousarray(self.pose, np.float64).copy()
        L.check(trk._lib.vh_fusion_step_sdf(self.table._h, trk._h, _ptr(depth_u16), _fp(self.k_inv), trk.dist_thres, trk.max_iters,
                                            _ptr(self.in_v), _ptr(self.in_n), _dp(pose.reshape(16)), C.byref(sys), C.byref(it)),
                "vh_fusion_step_sdf")
        self.pose = trk.pose = pose
        trk.last, trk.iterations = system_arrays(sys), int(it.value)
        self.frames += 1
        return self.pose

    def close(self):
        self.trk.close()


COLOR_WEIGHT = 0.1         # the prototype's and the literature's value (intensity 0..1 against metres); not tuned on this model
COLOR_THRES = 0.2          # a fifth of the intensity range: an occlusion edge or a highlight is no photometric row


class SdfColorTracking(SdfTracking):
    """SdfTracking with a photometric row beside the geometric one (vh_sdf_color_*; include/voxelhash.h, "tracking against the
    model's colour and shape"): SdfColorTracking(table); Align(input, rgba, start_pose) -> the camera -> world pose, with `rgba`
    the uint32 [H, W] colour image registered to the depth image.  A table without a colour volume, a view table or
    color_weight == 0 give SdfTracking's bits."""

    def __init__(self, table, color_weight: float = COLOR_WEIGHT, color_thres: float = COLOR_THRES, K=None,
                 dist_thres: float = DIST_THRES, max_iters: int = SDF_MAX_ITERS, width=None, height=None, stream=None):
        super().__init__(table, K, dist_thres=dist_thres, max_iters=max_iters, width=width, height=height, stream=stream)
        self.color_weight, self.color_thres = color_weight, color_thres

    def build_system(self, inp, rgba, pose):
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_sdf_color_build_system(self.table._h, self._h, _ptr(inp), _ptr(rgba), _fp(p), self.dist_thres,
                                                    self.color_weight, self.color_thres, C.byref(sys)), "vh_sdf_color_build_system")
        return system_arrays(sys)

    def residuals(self, inp, rgba, pose, points, sdf, gradient, color_residual, color_gradient):
        """The system, SdfTracking.residuals' three maps, and per pixel the photometric residual [H, W] (NaN without a
        photometric row) and the luminance gradient [H, W, 3] (0 without one), in place."""
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        sys = L.IcpSystem()
        L.check(self._lib.vh_sdf_color_residuals(self.table._h, self._h, _ptr(inp), _ptr(rgba), _fp(p), self.dist_thres,
                                                 self.color_weight, self.color_thres, _ptr(points), _ptr(sdf), _ptr(gradient),
                                                 _ptr(color_residual), _ptr(color_gradient), C.byref(sys)), "vh_sdf_color_residuals")
        return system_arrays(sys)

    def Align(self, inp, rgba, start_pose):
        """Up to max_iters joint rounds from `start_pose`; the result is kept in `pose`."""
        p = np.ascontiguousarray(np.asarray(start_pose, np.float64).reshape(16)).copy()
        sys, it = L.IcpSystem(), C.c_int32()
        L.check(self._lib.vh_sdf_color_align(self.table._h, self._h, _ptr(inp), _ptr(rgba), self.dist_thres, self.color_weight,
                                             self.color_thres, self.max_iters, _dp(p), C.byref(sys), C.byref(it)), "vh_sdf_color_align")
        self.pose, self.last, self.iterations = p.reshape(4, 4), system_arrays(sys), int(it.value)
        return self.pose


class SdfColorFusionLoop:
    """SdfFusionLoop for RGB-D frames: per uint16 depth image and uint32 colour image

        vh_preprocess(depth)                          -> input vertex map
        vh_sdf_color_align(input, rgba, start = pose) -> pose          (against the model's shape and colour as fused so far)
        vh_integrate_depth_color(pose, depth, rgba)   -> the model takes the frame

    all on the table's stream; the one host synchronisation of a frame is the Align's.  The first frame is integrated at
    `start_pose`.  `band` and `weight_max` are vh_integrate_color's."""

    def __init__(self, table, k_inv, band: float, weight_max: int = 255, color_weight: float = COLOR_WEIGHT,
                 color_thres: float = COLOR_THRES, K=None, stream=None, dist_thres: float = DIST_THRES, max_iters: int = SDF_MAX_ITERS):
        import torch
        self.table, self.W, self.H = table, table.width, table.height
        self.k_inv = np.ascontiguousarray(np.asarray(k_inv, np.float32).reshape(9))
        self.band, self.weight_max = float(band), int(weight_max)
        self.trk = SdfColorTracking(table, color_weight, color_thres, K, dist_thres=dist_thres, max_iters=max_iters, stream=stream)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.in_v, self.in_n = (torch.empty((self.H, self.W, 4), dtype=torch.float32, device=dev) for _ in range(2))
        self.stream = self.trk.stream_handle
        self.pose = None
        self.frames = 0

    def start(self, depth_u16, rgba, start_pose):
        self.pose = np.asarray(start_pose, np.float64).reshape(4, 4).copy()
        self.table.integrate_depth_color(self.pose.astype(np.float32), depth_u16, self.k_inv, rgba, self.band, self.weight_max)
        self.frames = 1
        return self.pose

    def track(self, depth_u16, rgba):
        """pre-process + Align only: the new pose (not yet integrated)."""
        from .hashtable import preprocess
        preprocess(depth_u16, self.k_inv, self.in_v, self.in_n, stream=self.stream)
        self.pose = self.trk.Align(self.in_v, rgba, self.pose)
        return self.pose

    def fuse(self, depth_u16, rgba):
        """integrate depth and colour at the current pose."""
        self.table.integrate_depth_color(self.pose.astype(np.float32), depth_u16, self.k_inv, rgba, self.band, self.weight_max)
        self.frames += 1

    def step(self, depth_u16, rgba):
        """track + fuse in one library call (vh_fusion_step_sdf_color)."""
        sys, it = L.IcpSystem(), C.c_int32()
        trk = self.trk
        pose = np.ascontiguousarray(self.pose, np.float64).copy()
        L.check(trk._lib.vh_fusion_step_sdf_color(self.table._h, trk._h, _ptr(depth_u16), _fp(self.k_inv), _ptr(rgba), trk.dist_thres,
                                                  trk.color_weight, trk.color_thres, trk.max_iters, self.band, self.weight_max,
                                                  _ptr(self.in_v), _ptr(self.in_n), _dp(pose.reshape(16)), C.byref(sys),
                                                  C.byref(it)), "vh_fusion_step_sdf_color")
        self.pose = trk.pose = pose
        trk.last, trk.iterations = system_arrays(sys), int(it.value)
        self.frames += 1
        return self.pose

    def close(self):
        self.trk.close()
