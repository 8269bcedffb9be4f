"""Host-side mirror of the reference's labeler interface on top of libgsx.so.

Same names, argument meaning and results as /root/reference/deep_learning_segmentation.py:
load_cameras (:17), project_gaussian (:43), assign_labels (:241) — except that assign_labels
takes its segmentation maps from a callable / directory instead of running a model, because the
2-D segmentation networks are outside this library.
"""
import ctypes as C
import json
import os

import numpy as np

from . import _lib
from ._lib import EDIT_TABLE_MAX, NO_SELECTION, Camera, RenderEdits, check

try:  # CPython binding of the per-view hand-over (csrc/gsxfast.c); without it the ctypes path below does the same
    from . import _gsxfast as _fast
except ImportError:
    _fast = None
if os.environ.get("GSX_NO_FAST_BINDING"):
    _fast = None


def camera_array(cameras):
    """ctypes array of gsx_camera from Camera structs and/or cameras.json dicts"""
    return (Camera * len(cameras))(*[c if isinstance(c, Camera) else Camera.from_dict(c) for c in cameras])


def load_cameras(camera_file):
    """cameras.json -> list of dicts (reference: deep_learning_segmentation.py:17-22)."""
    with open(camera_file, "r") as f:
        return json.load(f)


_SEG_TORCH_DT = {"torch.int32": _lib.GSX_SEG_I32, "torch.int64": _lib.GSX_SEG_I64, "torch.uint8": _lib.GSX_SEG_U8_LABELS}
_SEG_NP_DT = {np.dtype(np.int32): _lib.GSX_SEG_I32, np.dtype(np.int64): _lib.GSX_SEG_I64, np.dtype(np.uint8): _lib.GSX_SEG_U8_LABELS}


def _seg_map_arg(seg_map, packed_u8):
    """A class map as the library takes it -> (obj, GSX_SEG_* code, h, w, device): a C-contiguous 2-D numpy array, or with
    device=True a contiguous tensor on the GPU.  int32, int64 and uint8 go as they are, every other dtype is widened to int32;
    packed_u8: a uint8 map already holds label + 1.  (Once per view in a 10 ms run: the usual case - a contiguous array of a
    supported dtype - is passed through without a numpy call.)"""
    device = type(seg_map) is not np.ndarray and hasattr(seg_map, "data_ptr")   # a torch tensor
    if device:
        seg = seg_map.contiguous()
        if not seg.is_cuda:
            raise ValueError("tensor seg maps must live on the GPU; pass numpy arrays for host maps")
        dt = _SEG_TORCH_DT.get(str(seg.dtype))
        if dt is None:
            import torch
            seg, dt = seg.to(torch.int32), _lib.GSX_SEG_I32
    else:
        seg = seg_map if type(seg_map) is np.ndarray else np.asarray(seg_map)
        dt = _SEG_NP_DT.get(seg.dtype)
        if dt is None:
            seg, dt = seg.astype(np.int32, copy=False), _lib.GSX_SEG_I32
        if not seg.flags.c_contiguous:
            seg = np.ascontiguousarray(seg)
    if seg.ndim != 2:
        raise ValueError("seg_map must be 2-D")
    if packed_u8 and dt == _lib.GSX_SEG_U8_LABELS:
        dt = _lib.GSX_SEG_U8
    h, w = seg.shape
    return seg, dt, h, w, device


class _DeviceInts:
    """Zero-copy int32 view of device memory owned by libgsx (via __cuda_array_interface__)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(s) for s in shape), "typestr": "<i4", "data": (int(ptr), False), "version": 2}


def _scaled_camera(camera, w, h, image_size=None):
    """the camera with fx, fy scaled to a w x h frame from the (width, height) they refer to: image_size, or the camera's own"""
    cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
    iw, ih = (cam.width, cam.height) if image_size is None else (int(image_size[0]), int(image_size[1]))
    if (iw, ih) != (w, h) and iw > 0 and ih > 0:
        scaled = Camera()
        C.memmove(C.byref(scaled), C.byref(cam), C.sizeof(Camera))
        scaled.fx, scaled.fy, scaled.width, scaled.height = cam.fx * (w / iw), cam.fy * (h / ih), w, h
        cam = scaled
    return cam


class DepthFrame:
    """What Context.depth_view returns: total uint32, moment int64, surface_key int32, surface_index int32 (upload rows, -1 =
    no surface), all (height, width), row 0 on top, and the view's scale, offset with z_view = key * scale + offset.
    expected_z = moment / total * scale + offset, NaN where total == 0; surface_z, NaN where the pixel has no surface; both
    float64 (height, width), computed in numpy when first read.  total, moment and expected_z are None after a surface-only
    view."""

    def __init__(self, total, moment, surface_key, surface_index, scale, offset):
        self.total, self.moment, self.surface_key, self.surface_index = total, moment, surface_key, surface_index
        self.scale, self.offset = float(scale), float(offset)
        self._surface_z = self._expected_z = None

    @property
    def surface_z(self):
        if self._surface_z is None:
            self._surface_z = np.where(self.surface_index >= 0, self.surface_key.astype(np.float64) * self.scale + self.offset, np.nan)
        return self._surface_z

    @property
    def expected_z(self):
        if self._expected_z is None and self.total is not None and self.moment is not None:
            fed = self.total > 0
            mean = np.divide(self.moment.astype(np.float64), self.total.astype(np.float64), out=np.zeros(self.total.shape), where=fed)
            self._expected_z = np.where(fed, mean * self.scale + self.offset, np.nan)
        return self._expected_z


def depth_key_to_z(camera, width, height):
    """host only: (scale, offset) with z_view = key * scale + offset for the depth keys of the view (camera, width, height) -
    runSort's int32 keys, as depth_view and debug_render_pre report them (gsx_depth_key_to_z).  The camera is taken as given:
    scale fx, fy first where the frame is not the camera's own size (they do not enter the result)."""
    cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
    scale, offset = C.c_double(), C.c_double()
    check(_lib.lib().gsx_depth_key_to_z(C.byref(cam), int(width), int(height), C.byref(scale), C.byref(offset)))
    return scale.value, offset.value


class Context:
    """One GPU (gsx_ctx).  device: HIP ordinal; defaults to LOCAL_RANK or 0."""

    def __init__(self, device=None):
        self._lib = _lib.lib()
        if device is None:  # one process per GPU: LOCAL_RANK picks it (wrapping when ranks share a GPU in a rehearsal)
            device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, self._lib.gsx_device_count())
        h = C.c_void_p()
        check(self._lib.gsx_create(int(device), C.byref(h)))
        self.h = h
        self._vote_view_addr = C.cast(self._lib.gsx_vote_view, C.c_void_p).value   # for the CPython fast path
        self.device = int(device)
        self._keep_alive = []   # device maps handed to vote_view until the ctx stream has consumed them
        self._ext = None        # the ctx stream as torch sees it (segmap_from_*)
        self._lift_bins, self._lift_keep = 1, []   # columns of the lift table; the device map a lift view may still read
        self._assoc_shape = (2, 2)                 # the association table's shape, set by assoc_begin
        self._label_shape = None                   # (height, width) of the map at label_map_device()
        self._depth_shape = None                   # ... and of the maps at depth_surface_*_device()

    def close(self):
        if getattr(self, "h", None):
            self._lib.gsx_destroy(self.h)
            self.h = None
            self._ext = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, name, value):
        """Tuning knobs of gsx_set_option (spatial_sort, xcd_swizzle, vote_unroll); never change results."""
        check(self._lib.gsx_set_option(self.h, name.encode(), int(value)), self.h)

    def get_option(self, name):
        """gsx_get_option: the current value of an option that can be read back (early_vote, ...)."""
        out = C.c_int64(0)
        check(self._lib.gsx_get_option(self.h, name.encode(), C.byref(out)), self.h)
        return int(out.value)

    # -- scene ---------------------------------------------------------------------------------
    def upload_positions(self, positions):
        """positions: (N,3) float array, or a structured array with a 'position' field
        (the reference's `gaussians`, deep_learning_segmentation.py:33-38)."""
        if getattr(positions, "dtype", None) is not None and positions.dtype.names and "position" in positions.dtype.names:
            positions = positions["position"]
        pos = np.asarray(positions, dtype=np.float32)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("positions must have shape (N, 3)")
        x = np.ascontiguousarray(pos[:, 0])
        y = np.ascontiguousarray(pos[:, 1])
        z = np.ascontiguousarray(pos[:, 2])
        check(self._lib.gsx_upload_positions(self.h, len(pos), x.ctypes.data, y.ctypes.data, z.ctypes.data), self.h)
        self.n = len(pos)

    def upload_rows(self, rows, off_x, off_y, off_z):
        """AoS rows (e.g. PLY vertex records as a 2-D uint8 array or structured array)."""
        rows = np.ascontiguousarray(rows)
        check(self._lib.gsx_upload_positions_strided(self.h, len(rows), rows.ctypes.data, rows.strides[0], off_x, off_y,
                                                     off_z), self.h)
        self.n = len(rows)

    # -- projection probe ------------------------------------------------------------------------
    def project_one(self, position, camera):
        p = (C.c_float * 3)(*[float(v) for v in position])
        cam = Camera.from_dict(camera)
        x, y, vis = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._lib.gsx_project_one(self.h, p, C.byref(cam), C.byref(x), C.byref(y), C.byref(vis)), self.h)
        return (x.value, y.value) if vis.value else None

    def project_all(self, camera):
        cam = Camera.from_dict(camera)
        x = np.empty(self.n, np.int32)
        y = np.empty(self.n, np.int32)
        check(self._lib.gsx_project_all(self.h, C.byref(cam), x.ctypes.data, y.ctypes.data), self.h)
        return x, y

    # -- vote --------------------------------------------------------------------------------------
    def vote_begin(self, n_classes, first_view=0, total_views=255):
        self._keep_alive.clear()
        check(self._lib.gsx_vote_begin(self.h, n_classes, first_view, total_views), self.h)

    def vote_view(self, camera, seg_map, image_size=None, packed_u8=False):
        """seg_map: 2-D int array of labels (-1..n_classes-1; any integer dtype, as the reference accepts) on the host,
        or a torch tensor on this GPU.  image_size: (width, height) of the input image; defaults to the map's own size.
        packed_u8: a uint8 map already holds label+1 (0 = label -1), the library's own compact form.
        Host maps are range-checked here (ValueError); device maps when the labels are fetched."""
        cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
        if _fast is not None and type(seg_map) is np.ndarray and self.h is not None:
            # the usual case in C (csrc/gsxfast.c): a contiguous 2-D int32 / int64 / uint8 array; anything else is declined
            iw, ih = (-1, -1) if image_size is None else (int(image_size[0]), int(image_size[1]))
            rc = _fast.vote_view(self._vote_view_addr, self.h.value, C.addressof(cam), seg_map, packed_u8, iw, ih)
            if rc != _fast.DECLINED:
                check(rc, self.h)
                return
        seg, dt, h, w, device = _seg_map_arg(seg_map, packed_u8)
        iw, ih = (w, h) if image_size is None else (int(image_size[0]), int(image_size[1]))
        if device:
            check(self._lib.gsx_vote_view_device(self.h, C.byref(cam), seg.data_ptr(), dt, w, h, iw, ih), self.h)
            self._keep_alive.append(seg)   # the pack kernel runs asynchronously on the ctx stream
            return
        try:
            ptr = C.addressof(C.c_char.from_buffer(seg))   # 3x cheaper than seg.ctypes.data
        except (TypeError, ValueError):                    # a read-only or empty array
            ptr = seg.ctypes.data
        check(self._lib.gsx_vote_view(self.h, C.byref(cam), ptr, dt, w, h, iw, ih), self.h)

    def vote_views_device(self, cameras, seg_tensors, image_size=None, packed_u8=False):
        """Several device-resident maps of one shape and dtype in one call (gsx_vote_views_device: 16 maps per kernel
        launch).  seg_tensors: list of 2-D torch tensors on this GPU, or one 3-D tensor (views, H, W)."""
        ts = [t.contiguous() for t in seg_tensors]
        if not ts:
            return
        h, w = ts[0].shape
        dt = _SEG_TORCH_DT[str(ts[0].dtype)]   # (several maps of ONE supported dtype: nothing is widened here, unlike _seg_map_arg)
        if packed_u8 and dt == _lib.GSX_SEG_U8_LABELS:
            dt = _lib.GSX_SEG_U8
        if any(t.shape != ts[0].shape or t.dtype != ts[0].dtype or not t.is_cuda for t in ts):
            raise ValueError("vote_views_device: all maps must share shape and dtype and live on the GPU")
        cams = (Camera * len(ts))(*[c if isinstance(c, Camera) else Camera.from_dict(c) for c in cameras])
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        iw, ih = image_size if image_size is not None else (w, h)
        check(self._lib.gsx_vote_views_device(self.h, len(ts), cams, ptrs, dt, w, h, int(iw), int(ih)), self.h)
        self._keep_alive.extend(ts)

    def vote_rewind(self):
        check(self._lib.gsx_vote_rewind(self.h), self.h)

    def vote_finalize(self, to_host=True, out=None):
        """out: optional preallocated int32 array of N labels (saves the page faults of a fresh 12 MB array)."""
        if to_host and out is None:
            out = np.empty(self.n, np.int32)
        if to_host and (out.dtype != np.int32 or out.shape != (self.n,) or not out.flags.c_contiguous):
            raise ValueError("out must be a contiguous int32 array of N labels")
        try:
            check(self._lib.gsx_vote_finalize(self.h, out.ctypes.data if to_host else None), self.h)
        finally:
            self._keep_alive.clear()     # the stream has been synchronised
        return out if to_host else None

    def vote_flush(self):
        check(self._lib.gsx_vote_flush(self.h), self.h)

    def vote_tiebreak_keys(self):
        check(self._lib.gsx_vote_tiebreak_keys(self.h), self.h)

    def vote_labels_from_keys(self, to_host=True, out=None):
        if to_host and out is None:
            out = np.empty(self.n, np.int32)
        try:
            check(self._lib.gsx_vote_labels_from_keys(self.h, out.ctypes.data if to_host else None), self.h)
        finally:
            self._keep_alive.clear()
        return out if to_host else None

    def counts_device(self):
        n = C.c_int64()
        p = self._lib.gsx_vote_counts_device(self.h, C.byref(n))
        return p, n.value

    def keys_device(self):
        n = C.c_int64()
        p = self._lib.gsx_vote_keys_device(self.h, C.byref(n))
        return p, n.value

    def first_device(self):
        n = C.c_int64()
        p = self._lib.gsx_vote_first_device(self.h, C.byref(n))
        return p, n.value

    def slab_size(self):
        return self._lib.gsx_vote_slab_size(self.h)

    def vote_slab_reduce(self, recv_counts_ptr, recv_first_ptr):
        check(self._lib.gsx_vote_slab_reduce(self.h, C.c_void_p(recv_counts_ptr), C.c_void_p(recv_first_ptr)), self.h)

    def vote_flush_counts(self):
        check(self._lib.gsx_vote_flush_counts(self.h), self.h)

    def vote_slab_totals(self, recv_counts_ptr):
        check(self._lib.gsx_vote_slab_totals(self.h, C.c_void_p(recv_counts_ptr)), self.h)

    def cand_device(self):
        n = C.c_int64()
        p = self._lib.gsx_vote_cand_device(self.h, C.byref(n))
        return p, n.value

    def vote_tie_codes(self, cand_all_ptr):
        check(self._lib.gsx_vote_tie_codes(self.h, C.c_void_p(cand_all_ptr)), self.h)

    def codes_device(self):
        n = C.c_int64()
        p = self._lib.gsx_vote_codes_device(self.h, C.byref(n))
        return p, n.value

    def vote_tie_resolve(self, recv_codes_ptr):
        check(self._lib.gsx_vote_tie_resolve(self.h, C.c_void_p(recv_codes_ptr)), self.h)

    def vote_labels_from_sorted(self, sorted_ptr, to_host=True, out=None):
        if to_host and out is None:
            out = np.empty(self.n, np.int32)
        try:
            check(self._lib.gsx_vote_labels_from_sorted(self.h, C.c_void_p(sorted_ptr), out.ctypes.data if to_host else None),
                  self.h)
        finally:
            self._keep_alive.clear()
        return out if to_host else None

    def kmeans(self, points, colors, k, init_index, max_iter=100, tol=1e-4):
        """k_means_with_color (3D_clustering/k_means.py:107-151) with injected initial rows.
        Returns (centroids float32 (k, 6), labels int32 (n,), iterations, converged)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        col = np.ascontiguousarray(colors, np.float32).reshape(-1, 3)
        if len(pts) != len(col):
            raise ValueError("points and colors differ in length")
        init = np.ascontiguousarray(init_index, np.int64)
        if init.shape != (int(k),):
            raise ValueError("init_index must hold k row indices")
        labels = np.empty(len(pts), np.int32)
        cent = np.empty((int(k), 6), np.float32)
        iters, conv = C.c_int32(0), C.c_int32(0)
        check(self._lib.gsx_kmeans(self.h, len(pts), pts.ctypes.data, col.ctypes.data, int(k), init.ctypes.data, int(max_iter),
                                   float(tol), labels.ctypes.data, cent.ctypes.data, C.byref(iters), C.byref(conv)), self.h)
        return cent, labels, int(iters.value), bool(conv.value)

    # -- region-growing labeler (3D_clustering/region_growing.py; csrc/normals.hip, csrc/region_grow.cpp) --------------------
    def normals(self, points, k):
        """compute_normals + compute_residuals (region_growing.py:78-163) over the exact k nearest points of every point.
        Returns (normals float64 (n, 3), residuals float64 (n,))."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        nrm = np.empty((len(pts), 3), np.float64)
        res = np.empty(len(pts), np.float64)
        check(self._lib.gsx_normals(self.h, len(pts), pts.ctypes.data, int(k), nrm.ctypes.data, res.ctypes.data), self.h)
        return nrm, res

    def debug_normals_moments(self, points, k):
        """test hook: (centroid (n, 3), covariance (n, 3, 3)) of every point's k nearest points, as gsx_normals forms them"""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        mo = np.empty((len(pts), 9), np.float64)
        check(self._lib.gsx_debug_normals_moments(self.h, len(pts), pts.ctypes.data, int(k), mo.ctypes.data), self.h)
        cov = mo[:, [3, 4, 5, 4, 6, 7, 5, 7, 8]].reshape(-1, 3, 3)
        return mo[:, :3].copy(), cov

    def knn(self, points, k):
        """kd_tree.query(points[i], k)[1] for every i (region_growing.py:205): int32 (n, k), ascending distance, then index."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        idx = np.empty((len(pts), max(int(k), 0)), np.int32)
        check(self._lib.gsx_knn(self.h, len(pts), pts.ctypes.data, int(k), idx.ctypes.data), self.h)
        return idx

    def region_growing(self, points, k_normals=2000, k=10, residual_threshold=0.1, angle_threshold=0.05):
        """The reference's run (region_growing.py:270-278).  Returns (labels int32 (n,), normals, residuals, n_regions);
        label 0 is the largest region."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        labels = np.empty(len(pts), np.int32)
        nrm = np.empty((len(pts), 3), np.float64)
        res = np.empty(len(pts), np.float64)
        nreg = C.c_int32(0)
        check(self._lib.gsx_region_growing(self.h, len(pts), pts.ctypes.data, int(k_normals), int(k), float(residual_threshold),
                                           float(angle_threshold), labels.ctypes.data, nrm.ctypes.data, res.ctypes.data,
                                           C.byref(nreg)), self.h)
        return labels, nrm, res, int(nreg.value)

    # -- label clean-up (csrc/smooth.hip): majority filter over the k nearest neighbours, hole filling ----------------------
    def _smooth(self, call, n, labels, rounds, min_votes, ignore_label, fill_only, return_support):
        if fill_only and ignore_label is None:
            raise ValueError("fill_only needs an ignore_label: the label that marks a hole")
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if len(lab) != n:
            raise ValueError("labels must hold one entry per point")
        flags = (_lib.GSX_SMOOTH_IGNORE if ignore_label is not None else 0) | (_lib.GSX_SMOOTH_FILL_ONLY if fill_only else 0)
        out = np.empty(n, np.int32)
        sup = np.empty(n, np.int32) if return_support else None
        changed = np.zeros(max(int(rounds), 0), np.int64)
        done = C.c_int32(0)
        check(call(lab.ctypes.data, int(rounds), int(min_votes), int(ignore_label or 0), flags, out.ctypes.data,
                   sup.ctypes.data if return_support else None, changed.ctypes.data, C.byref(done)), self.h)
        self.smooth_rounds_done = int(done.value)
        changed = [int(v) for v in changed]
        return (out, changed, sup) if return_support else (out, changed)

    def smooth_labels(self, points, labels, k=16, rounds=1, min_votes=1, ignore_label=None, fill_only=False, return_support=False):
        """gsx_smooth_labels (include/gsx.h): `rounds` Jacobi rounds of the majority filter over every point's exact k nearest
        neighbours.  ignore_label: neighbours with this label cast no vote (None: every neighbour votes); fill_only: only points
        whose label is ignore_label change.  Returns (labels int32 (n,), changed per round - a list of `rounds` counts, 0 behind
        the round that changed nothing) plus support int32 (n,) with return_support; self.smooth_rounds_done = rounds executed."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        return self._smooth(lambda *a: self._lib.gsx_smooth_labels(self.h, len(pts), pts.ctypes.data, a[0], int(k), *a[1:]), len(pts), labels,
                            rounds, min_votes, ignore_label, fill_only, return_support)

    def smooth_labels_lists(self, knn, labels, rounds=1, min_votes=1, ignore_label=None, fill_only=False, return_support=False, k=None):
        """gsx_smooth_labels_lists: the same rounds over neighbour lists int32 (n, k <= 64) - or, with knn None, over the
        device lists the last knn / region_growing call left on this context (their k must be given)."""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if knn is None:
            if k is None:
                raise ValueError("knn is None: k of the context's device lists is needed")
            nb, kk = None, int(k)
        else:
            nb = np.ascontiguousarray(knn, np.int32)
            if nb.ndim != 2 or len(nb) != len(lab):
                raise ValueError("knn (n, k) and labels (n,) must agree in n")
            kk = nb.shape[1]
        return self._smooth(lambda *a: self._lib.gsx_smooth_labels_lists(self.h, len(lab), kk, None if nb is None else nb.ctypes.data, *a),
                            len(lab), lab, rounds, min_votes, ignore_label, fill_only, return_support)

    # -- classes into objects (csrc/split.hip): connected components of every label over the k-nearest-neighbour graph --------
    def _split(self, call, n, labels, max_dist, min_size, max_instances, ignore_label, return_components):
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if len(lab) != n:
            raise ValueError("labels must hold one entry per point")
        flags = _lib.GSX_SPLIT_IGNORE if ignore_label is not None else 0
        out, comp = np.empty(n, np.int32), np.empty(n, np.int32) if return_components else None
        t_label, t_size, t_rep = np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.int32)
        m, ncomp = C.c_int32(0), C.c_int64(0)
        check(call(lab.ctypes.data, float("inf") if max_dist is None else float(max_dist), int(min_size), int(max_instances),
                   int(ignore_label or 0), flags, out.ctypes.data, comp.ctypes.data if return_components else None, t_label.ctypes.data,
                   t_size.ctypes.data, t_rep.ctypes.data, C.byref(m), C.byref(ncomp)), self.h)
        self.split_components = int(ncomp.value)
        m = int(m.value)
        table = {"label": t_label[:m].copy(), "size": t_size[:m].copy(), "rep": t_rep[:m].copy()}
        return (out, table, comp) if return_components else (out, table)

    def split_labels(self, points, labels, k=16, max_dist=None, min_size=1, max_instances=0, ignore_label=None, return_components=False):
        """gsx_split_labels (include/gsx.h): the connected components of every label over the exact k-nearest-neighbour graph,
        as instance ids - the largest component is 0; components below min_size or behind max_instances, and points whose label
        is ignore_label, get -1.  max_dist: neighbours farther apart are not joined (None: no cut).  Returns (labels int32 (n,),
        table) - table = {"label", "size", "rep"}, one entry per instance - plus the representatives int32 (n,) with
        return_components; self.split_components = components before the size filter."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        return self._split(lambda *a: self._lib.gsx_split_labels(self.h, len(pts), pts.ctypes.data, a[0], int(k), *a[1:]), len(pts), labels,
                           max_dist, min_size, max_instances, ignore_label, return_components)

    def split_labels_lists(self, knn, labels, points=None, max_dist=None, min_size=1, max_instances=0, ignore_label=None,
                           return_components=False, k=None):
        """gsx_split_labels_lists: the same over neighbour lists int32 (n, k <= 64) - or, with knn None, over the device lists
        the last knn / region_growing / smooth_labels / split_labels call left on this context (their k must be given).  points
        are needed only with a max_dist."""
        lab = np.ascontiguousarray(labels, np.int32).reshape(-1)
        if knn is None:
            if k is None:
                raise ValueError("knn is None: k of the context's device lists is needed")
            nb, kk = None, int(k)
        else:
            nb = np.ascontiguousarray(knn, np.int32)
            if nb.ndim != 2 or len(nb) != len(lab):
                raise ValueError("knn (n, k) and labels (n,) must agree in n")
            kk = nb.shape[1]
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            if len(pts) != len(lab):
                raise ValueError("points (n, 3) and labels (n,) must agree in n")
        elif max_dist is not None and np.isfinite(max_dist):
            raise ValueError("max_dist needs points")
        return self._split(lambda *a: self._lib.gsx_split_labels_lists(self.h, len(lab), kk, None if nb is None else nb.ctypes.data,
                                                                       None if pts is None else pts.ctypes.data, *a),
                           len(lab), lab, max_dist, min_size, max_instances, ignore_label, return_components)

    # -- exchange protocol v4 (see include/gsx.h) ------------------------------------------------------------------------
    def vote_num_views(self):
        return int(self._lib.gsx_vote_num_views(self.h))

    def vote_export(self, reserve_bytes=0, blobs=True):
        """-> (pool device pointer, bytes in use, blobs uint8 (views, 256) or None)."""
        nv = self.vote_num_views()
        b = np.empty((nv, 256), np.uint8) if blobs else None
        ptr, used = C.c_void_p(), C.c_int64()
        check(self._lib.gsx_vote_export(self.h, int(reserve_bytes), b.ctypes.data if blobs and nv else None, C.byref(ptr),
                                        C.byref(used)), self.h)
        return ptr.value, int(used.value), b

    def vote_pool_bytes(self):
        return int(self._lib.gsx_vote_pool_bytes(self.h))

    def vote_link_bytes(self):
        """bytes of host maps sent over PCIe since vote_begin (compact records, or maps in pool form)"""
        return int(self._lib.gsx_vote_link_bytes(self.h))

    def vote_early_views(self):
        """views of this run that were voted on the second stream while the rest was handed over (0: one-piece vote)"""
        return int(self._lib.gsx_vote_early_views(self.h))

    def vote_import(self, part_views, part_offsets, blobs, pool_all_ptr, pool_all_bytes):
        pv = np.ascontiguousarray(part_views, np.int32)
        po = np.ascontiguousarray(part_offsets, np.int64)
        bl = np.ascontiguousarray(blobs, np.uint8)
        check(self._lib.gsx_vote_import(self.h, len(pv), pv.ctypes.data, po.ctypes.data, bl.ctypes.data if bl.size else None,
                                        C.c_void_p(pool_all_ptr), int(pool_all_bytes)), self.h)

    def vote_import_uniform(self, part_views, part_offsets, cams, map_size, image_size, pool_all_ptr, pool_all_bytes):
        """gsx_vote_import_uniform: cams = the cameras of ALL views in global order (Camera structs, a ctypes array of them, or
        dicts); map_size / image_size = (width, height) shared by every view of the run."""
        pv = np.ascontiguousarray(part_views, np.int32)
        po = np.ascontiguousarray(part_offsets, np.int64)
        arr = cams if isinstance(cams, C.Array) else camera_array(cams)
        check(self._lib.gsx_vote_import_uniform(self.h, len(pv), pv.ctypes.data, po.ctypes.data, C.addressof(arr) if len(arr) else None,
                                                int(map_size[0]), int(map_size[1]), int(image_size[0]), int(image_size[1]),
                                                C.c_void_p(pool_all_ptr), int(pool_all_bytes)), self.h)

    def vote_import_undo(self):
        check(self._lib.gsx_vote_import_undo(self.h), self.h)

    def vote_map_stride(self, map_size):
        """gsx_vote_map_stride: bytes from one staged map of map_size = (width, height) to the next (after vote_begin)."""
        out = C.c_int64(0)
        check(self._lib.gsx_vote_map_stride(self.h, int(map_size[0]), int(map_size[1]), C.byref(out)), self.h)
        return int(out.value)

    def vote_views_match_uniform(self, cams, map_size, image_size):
        """gsx_vote_views_match_uniform: are this context's own views exactly the views of `cams` (in order) with this map and
        image size, as vote_import_uniform would derive them?"""
        arr = cams if isinstance(cams, C.Array) else camera_array(cams)
        out = C.c_int32(0)
        check(self._lib.gsx_vote_views_match_uniform(self.h, len(arr), C.addressof(arr) if len(arr) else None, int(map_size[0]),
                                                     int(map_size[1]), int(image_size[0]), int(image_size[1]), C.byref(out)), self.h)
        return bool(out.value)

    def vote_slab_labels(self, slab, slabs):
        """-> slab size S; the slab's labels (Morton order) are the first S words at keys_device()."""
        sn = C.c_int64()
        check(self._lib.gsx_vote_slab_labels(self.h, int(slab), int(slabs), C.byref(sn)), self.h)
        return int(sn.value)

    def host_threads(self):
        return int(self._lib.gsx_host_threads(self.h))

    def vote_culled(self, reset=False):
        """(wave, view) pairs skipped by the wave culling so far (gsx_vote_culled)."""
        out = C.c_int64(0)
        check(self._lib.gsx_vote_culled(self.h, C.byref(out), 1 if reset else 0), self.h)
        return int(out.value)

    def debug_filter_check(self):
        """gsx_debug_filter_check: [max relative error of v_rcp_f32 in units of 2^-24, fract x 8, floor-convert x 8]."""
        out = np.zeros(17, np.float64)
        check(self._lib.gsx_debug_filter_check(self.h, out.ctypes.data), self.h)
        return out

    def debug_planes(self, bins):
        cnt = np.empty((bins, self.n), np.uint16)
        fv = np.empty((bins, self.n), np.uint16)
        check(self._lib.gsx_vote_debug_planes(self.h, cnt.ctypes.data, fv.ctypes.data), self.h)
        return cnt, fv

    # -- rasterizer ---------------------------------------------------------------------------------
    def upload_splats(self, xyz, scale, rot, opacity, f_dc, labels=None):
        """3DGS PLY attributes as float arrays (see include/gsx.h).  scale/opacity may be None."""
        f32 = lambda a, w: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, w))
        xyz, scale, rot, f_dc = f32(xyz, 3), f32(scale, 3), f32(rot, 4), f32(f_dc, 3)
        opacity = None if opacity is None else np.ascontiguousarray(np.asarray(opacity, dtype=np.float32).reshape(-1))
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
        n = len(xyz)
        for a in (scale, rot, opacity, f_dc, lab):
            if a is not None and len(a) != n:
                raise ValueError("all splat attribute arrays must have the same number of rows")
        ptr = lambda a: None if a is None else a.ctypes.data
        check(self._lib.gsx_upload_splats(self.h, n, ptr(xyz), ptr(scale), ptr(rot), ptr(opacity), ptr(f_dc), ptr(lab)),
              self.h)
        self.n_splats = n

    def upload_sh(self, f_rest, degree):
        """Switch the colour path to float spherical harmonics of `degree` (see gsx_upload_sh)."""
        k1 = (degree + 1) ** 2 - 1
        fr = None
        if k1:
            fr = np.ascontiguousarray(np.asarray(f_rest, dtype=np.float32).reshape(self.n_splats, 3 * k1))
        check(self._lib.gsx_upload_sh(self.h, None if fr is None else fr.ctypes.data, int(degree)), self.h)

    def set_render_edits(self, selected=None, selection_mode=False, colours=None, custom_colour=None, displacements=None,
                         hidden=()):
        """Label edits of the viewer (gsx_render_set_edits) for every following frame, until clear_render_edits() or the
        next upload_splats: `selected` + `selection_mode` highlight a label red, `colours` {label: rgb} recolours labels
        (mix 0.6), `custom_colour` rgb replaces the selected label's colour, `displacements` {label: xyz} moves labels
        (drawing only: depth order and hit_test stay), `hidden` labels are drawn with alpha 0.  A dict's insertion order
        is the table order, as the viewer's Map iterates; at most 100 entries each."""
        e = RenderEdits()
        e.selection_mode = 1 if selection_mode else 0
        e.selected_label = NO_SELECTION if selected is None else int(selected)
        if custom_colour is not None:
            e.enable_custom_color = 1
            for k, v in enumerate(np.asarray(custom_colour, np.float32).reshape(3)):
                e.custom_color[k] = v
        colours, displacements = dict(colours or {}), dict(displacements or {})
        e.num_colors, e.num_displacements = len(colours), len(displacements)  # (> 100: the library says so)
        for i, (label, rgb) in enumerate(list(colours.items())[:EDIT_TABLE_MAX]):
            e.color_labels[i] = int(label)
            e.colors[3 * i:3 * i + 3] = [float(v) for v in np.asarray(rgb, np.float32).reshape(3)]
        for i, (label, xyz) in enumerate(list(displacements.items())[:EDIT_TABLE_MAX]):
            e.displacement_labels[i] = int(label)
            e.displacements[3 * i:3 * i + 3] = [float(v) for v in np.asarray(xyz, np.float32).reshape(3)]
        e.enable_displacement = 1 if displacements else 0  # gs.js:919: displacementMap.size > 0
        hid = np.ascontiguousarray(list(hidden), dtype=np.int32)
        e.num_hidden = len(hid)
        e.hidden_labels = hid.ctypes.data if len(hid) else None
        check(self._lib.gsx_render_set_edits(self.h, C.byref(e)), self.h)

    def clear_render_edits(self):
        check(self._lib.gsx_render_set_edits(self.h, None), self.h)

    def render_num_hidden(self):
        """Splats the current edit state hides."""
        return self._lib.gsx_render_num_hidden(self.h)

    def render_view(self, camera, width, height, to_host=True):
        """One frame of the viewer's pipeline -> (height, width, 4) float32 premultiplied RGBA."""
        cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
        out = np.empty((height, width, 4), np.float32) if to_host else None
        check(self._lib.gsx_render_view(self.h, C.byref(cam), int(width), int(height), out.ctypes.data if to_host else None),
              self.h)
        return out

    def render_views(self, cameras, width, height, to_host=True):
        """Several frames of one size, up to four in flight on HIP streams of their own (gsx_render_views, option
        render_frames) -> (n, height, width, 4) float32, or None with to_host=False.  Same pixels as render_view, about half
        as many views per second again."""
        cams = (Camera * len(cameras))(*[c if isinstance(c, Camera) else Camera.from_dict(c) for c in cameras])
        out = np.empty((len(cameras), height, width, 4), np.float32) if to_host else None
        ptrs = (C.c_void_p * len(cameras))(*[out[k].ctypes.data for k in range(len(cameras))]) if to_host else None
        check(self._lib.gsx_render_views(self.h, len(cameras), cams, int(width), int(height), ptrs), self.h)
        return out

    def render_num_pairs(self):
        return self._lib.gsx_render_num_pairs(self.h)

    def render_num_pairs_consumed(self):
        return self._lib.gsx_render_num_pairs_consumed(self.h)

    # -- lifting labeler (include/gsx.h: gsx_lift_*) ------------------------------------------------
    def lift_begin(self, n_classes):
        """Start a lift run on the splats of upload_splats: a zeroed n x (n_classes + 1) table of blend weights."""
        self._lift_keep = []
        self._lift_bins = int(n_classes) + 1
        check(self._lib.gsx_lift_begin(self.h, int(n_classes)), self.h)

    def lift_view(self, camera, seg_map, image_size=None, packed_u8=False):
        """Lift one class map (2-D, labels -1..n_classes-1; a numpy array on the host or a torch tensor on this GPU) through
        the frame gsx_render_view draws from `camera` at the MAP's size.  image_size: (width, height) the camera's fx, fy
        refer to (default: the camera's own width, height); they are scaled by map size / image size, which is the caller's
        job at the C level.  Host maps are range-checked here (ValueError); device maps when the table is fetched."""
        seg, dt, h, w, device = _seg_map_arg(seg_map, packed_u8)
        cam = _scaled_camera(camera, w, h, image_size)
        if device:
            check(self._lib.gsx_lift_view_device(self.h, C.byref(cam), seg.data_ptr(), dt, w, h), self.h)
            self._lift_keep = [seg]          # the call waits for the frame: the previous map has been read
        else:
            check(self._lib.gsx_lift_view(self.h, C.byref(cam), seg.ctypes.data, dt, w, h), self.h)

    def lift_num_views(self):
        return self._lib.gsx_lift_num_views(self.h)

    def lift_num_atomics(self):
        """64-bit global atomics the lifting kernel issued for the last view"""
        return self._lib.gsx_lift_num_atomics(self.h)

    def lift_finalize(self, min_weight=0.0, return_share=False):
        """-> int32 labels in upload order (and the winner's share of each row as float64)"""
        n = self._lib.gsx_num_splats(self.h)
        labels = np.empty(n, np.int32)
        share = np.empty(n, np.float64) if return_share else None
        check(self._lib.gsx_lift_finalize(self.h, float(min_weight), labels.ctypes.data, None if share is None else share.ctypes.data),
              self.h)
        return (labels, share) if return_share else labels

    def lift_table(self):
        """-> uint64 (n, n_classes + 1), rows in upload order, column = label + 1, in units of 1 / 2^20"""
        table = np.empty((self._lib.gsx_num_splats(self.h), self._lift_bins), np.uint64)
        check(self._lib.gsx_lift_table(self.h, table.ctypes.data), self.h)
        return table

    # -- label frames (include/gsx.h: gsx_label_*) --------------------------------------------------
    def label_view(self, camera, width, height, n_classes, min_weight=0.0, planes=None, to_host=True, return_weights=False):
        """The labels given to upload_splats as the class map of the view `camera` draws at width x height: per pixel the label
        whose splats hold the largest share of the frame's alpha there, -1 where the total is under max(1, ceil(min_weight *
        2^20)) units of 1 / 2^20 (gsx_label_view).  The camera's fx, fy refer to its own width, height and are scaled to the
        frame as lift_view scales them to a map.  -> int32 (height, width), row 0 on top; with to_host=False nothing (the map
        stays at label_map_device()).  return_weights: also uint32 (weight, total), the winner's sum and the pixel's total.
        planes: labels whose summed weights are wanted -> also uint32 (len(planes), height, width).  The extras follow the
        map in the order (map, weight, total, planes); with to_host=False they start the tuple."""
        w, h = int(width), int(height)
        cam = _scaled_camera(camera, w, h)
        shape = (max(h, 0), max(w, 0))
        out = np.empty(shape, np.int32) if to_host else None
        weight = np.empty(shape, np.uint32) if return_weights else None
        total = np.empty(shape, np.uint32) if return_weights else None
        want = None if planes is None else np.ascontiguousarray(planes, dtype=np.int32).reshape(-1)
        n_planes = 0 if want is None else len(want)
        stack = np.empty((n_planes,) + shape, np.uint32) if 0 < n_planes <= 256 else None
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        check(self._lib.gsx_label_view(self.h, C.byref(cam), w, h, int(n_classes), float(min_weight), n_planes, ptr(want), ptr(out),
                                       ptr(weight), ptr(total), ptr(stack)), self.h)
        self._label_shape = (h, w)
        res = ([out] if to_host else []) + ([weight, total] if return_weights else []) + ([stack] if want is not None else [])
        return None if not res else res[0] if len(res) == 1 else tuple(res)

    def label_map_device(self):
        """The map of the last label_view as an int32 (height, width) torch tensor on this GPU: a zero-copy view of memory the
        context owns, written on the ctx stream (label_view has waited for it), valid until the next label_view or close().
        A class map for label_map_tables, vote_view and lift_view."""
        import torch
        p = self._lib.gsx_label_map_device(self.h)
        if not p or self._label_shape is None:
            raise RuntimeError("label_map_device: no label_view yet")
        h, w = self._label_shape
        return torch.as_tensor(_DeviceInts(p, (h, w)), device=torch.device("cuda", self.device))

    def label_num_passes(self):
        """walks of a tile's list summed over the tiles of the last label_view: ceil(labels in the list / window) per tile"""
        return self._lib.gsx_label_num_passes(self.h)

    def label_num_single_tiles(self):
        """tiles of the last label_view whose list held exactly one label"""
        return self._lib.gsx_label_num_single_tiles(self.h)

    # -- depth frames (include/gsx.h: gsx_depth_*) --------------------------------------------------
    def depth_view(self, camera, width, height, quantile=0.5, to_host=True, surface_only=False):
        """Per pixel of the view `camera` draws at width x height: the blend's expected depth and the surface, the first
        fragment at which the accumulated alpha reaches `quantile` (gsx_depth_view).  The camera's fx, fy are scaled to the
        frame as label_view scales them.  -> DepthFrame; surface_only: total, moment and expected_z stay None and a tile
        stops at its last surface (the surface maps are the same bits); to_host=False: nothing is copied, the maps stay at
        depth_surface_index_device() / depth_surface_key_device() - the sums have no device form, so this is a surface-only
        walk as well - and None is returned."""
        cam = _scaled_camera(camera, int(width), int(height))
        w, h = int(width), int(height)
        shape = (max(h, 0), max(w, 0))
        full = to_host and not surface_only
        total = np.empty(shape, np.uint32) if full else None
        moment = np.empty(shape, np.int64) if full else None
        key = np.empty(shape, np.int32) if to_host else None
        index = np.empty(shape, np.int32) if to_host else None
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        check(self._lib.gsx_depth_view(self.h, C.byref(cam), w, h, float(quantile), ptr(total), ptr(moment), ptr(key), ptr(index)),
              self.h)
        self._depth_shape = (h, w)
        if not to_host:
            return None
        scale, offset = depth_key_to_z(cam, w, h)
        return DepthFrame(total, moment, key, index, scale, offset)

    def _depth_map_device(self, fn, what):
        import torch
        p = fn(self.h)
        if not p or self._depth_shape is None:
            raise RuntimeError(f"{what}: no depth_view since the last upload_splats")
        return torch.as_tensor(_DeviceInts(p, self._depth_shape), device=torch.device("cuda", self.device))

    def depth_surface_index_device(self):
        """The surface's upload rows (-1: none) of the last depth_view as an int32 (height, width) torch tensor on this GPU: a
        zero-copy view of memory the context owns, valid until the next depth_view, upload_splats or close()."""
        return self._depth_map_device(self._lib.gsx_depth_surface_index_device, "depth_surface_index_device")

    def depth_surface_key_device(self):
        """... and the surface's depth keys (0 where there is none)"""
        return self._depth_map_device(self._lib.gsx_depth_surface_key_device, "depth_surface_key_device")

    def depth_num_surface(self):
        """pixels of the last depth_view with a surface"""
        return self._lib.gsx_depth_num_surface(self.h)

    def pick(self, x, y):
        """The surface of the LAST depth_view under the canvas point (x, y), y from the bottom as hit_test takes it ->
        (label or -999999, upload row or -1, view-space z or NaN).  Renders nothing (gsx_depth_pick)."""
        label, index, z = C.c_int32(), C.c_int64(), C.c_double()
        check(self._lib.gsx_depth_pick(self.h, float(x), float(y), C.byref(label), C.byref(index), C.byref(z)), self.h)
        return label.value, index.value, z.value

    # -- instance association (include/gsx.h: gsx_assoc_*) ------------------------------------------
    def assoc_begin(self, max_segments=254, max_instances=255, min_overlap=0.3, min_size=1):
        """Start an association run on the Gaussians of upload_positions: maps with segment ids -1 .. max_segments - 1 per
        view become maps of at most max_instances global instance ids."""
        check(self._lib.gsx_assoc_begin(self.h, int(max_segments), int(max_instances), float(min_overlap), int(min_size)), self.h)
        self._assoc_shape = (int(max_segments) + 1, int(max_instances) + 1)

    def assoc_view(self, camera, seg_map, image_size=None, packed_u8=False):
        """Associate one view's segment map (2-D; a numpy array on the host or a torch tensor on this GPU) with the run's
        instances -> (remap int32 (max_segments,), map_dev): remap[s] is the global instance of segment s or -1, map_dev the
        relabelled map as an int32 torch tensor on this GPU, a class map for vote_view / lift_view.  image_size as in
        vote_view.  A value outside [-1, max_segments - 1] raises ValueError and leaves the run as it was."""
        import torch
        cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
        seg, dt, h, w, device = _seg_map_arg(seg_map, packed_u8)
        iw, ih = (w, h) if image_size is None else (int(image_size[0]), int(image_size[1]))
        remap = np.empty(self._assoc_shape[0] - 1, np.int32)
        out = torch.empty((h, w), dtype=torch.int32, device=torch.device("cuda", self.device))
        # the ctx stream behind torch's: the producer of a device map, and whoever last used the block `out` was given
        self._seg_enter()
        fn, ptr = (self._lib.gsx_assoc_view_device, seg.data_ptr()) if device else (self._lib.gsx_assoc_view, seg.ctypes.data)
        check(fn(self.h, C.byref(cam), ptr, dt, w, h, iw, ih, remap.ctypes.data, out.data_ptr()), self.h)   # waits for its kernels
        return remap, out

    def assoc_num_views(self):
        return self._lib.gsx_assoc_num_views(self.h)

    def assoc_num_instances(self):
        """G: the global instances opened so far"""
        return self._lib.gsx_assoc_num_instances(self.h)

    def assoc_num_dropped(self):
        """segments that matched no instance when max_instances were already open"""
        return self._lib.gsx_assoc_num_dropped(self.h)

    def assoc_ids(self):
        """-> int32 (n,), upload order: the instance each Gaussian was first given, -1 = none"""
        gid = np.empty(int(self._lib.gsx_num_gaussians(self.h)), np.int32)
        check(self._lib.gsx_assoc_ids(self.h, gid.ctypes.data), self.h)
        return gid

    def assoc_table(self):
        """-> uint32 (max_segments + 1, max_instances + 1): the last view's table, row = segment + 1, column = instance + 1"""
        table = np.empty(self._assoc_shape, np.uint32)
        check(self._lib.gsx_assoc_table(self.h, table.ctypes.data), self.h)
        return table

    def hit_test(self, camera, width, height, x, y):
        """performHitTesting (gs.js:361-395) -> (label or -999999, importance-order row or -1)."""
        cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
        label, index = C.c_int32(), C.c_int64()
        check(self._lib.gsx_hit_test(self.h, C.byref(cam), int(width), int(height), float(x), float(y), C.byref(label),
                                     C.byref(index)), self.h)
        return label.value, index.value

    def render_debug(self, buckets=False):
        """(buffer (n,32) u8, order (n,) u32, texdata (8n,) u32[, buckets (n,) u32]) — test hooks."""
        n = self.n_splats
        buf = np.empty((n, 32), np.uint8)
        order = np.empty(n, np.uint32)
        tex = np.empty(8 * n, np.uint32)
        bk = np.empty(n, np.uint32) if buckets else None
        check(self._lib.gsx_render_debug(self.h, buf.ctypes.data, order.ctypes.data, tex.ctypes.data,
                                         bk.ctypes.data if buckets else None), self.h)
        return (buf, order, tex, bk) if buckets else (buf, order, tex)

    def debug_render_scene(self):
        """(labels (n,) i32 exact, in importance order; SH planes (K, 3, n) f32 or None while the SH colour is off; degree or
        -1) — test hook, gsx_debug_render_scene.  The row count is the library's (gsx_num_splats)."""
        n = self._lib.gsx_num_splats(self.h)
        deg = C.c_int32(-2)
        check(self._lib.gsx_debug_render_scene(self.h, None, None, C.byref(deg)), self.h)
        labels = np.empty(n, np.int32)
        sh = np.empty(((deg.value + 1) ** 2, 3, n), np.float32) if deg.value >= 0 else None
        check(self._lib.gsx_debug_render_scene(self.h, labels.ctypes.data, None if sh is None else sh.ctypes.data, None), self.h)
        return labels, sh, deg.value

    def debug_render_pre(self, cameras, width, height, multi=False, compact=True):
        """The rasterizer's per-splat pre pass and depth-bucket kernel for 1..6 cameras (test hook, gsx_debug_render_pre; multi:
        one launch of the several-view kernel instead of one launch per view) -> per view a dict: depth (n,) i32, rect (n,) u32,
        rec (n,12) f32 (0xFF bytes where no record was written), pre (4,) i32, bucket, key, rect_bucket (n,) u32, dropped int."""
        n, nv = self.n_splats, len(cameras)
        cams = (Camera * nv)(*[c if isinstance(c, Camera) else Camera.from_dict(c) for c in cameras])
        outs = [dict(depth=np.empty(n, np.int32), rect=np.empty(n, np.uint32), rec=np.empty((n, 12), np.float32),
                     pre=np.empty(4, np.int32), bucket=np.empty(n, np.uint32), key=np.empty(n, np.uint32),
                     rect_bucket=np.empty(n, np.uint32), dropped=np.empty(1, np.int32)) for _ in range(nv)]
        fields = ("depth", "rect", "rec", "pre", "bucket", "key", "rect_bucket", "dropped")
        ptrs = (C.c_void_p * (len(fields) * nv))(*[o[f].ctypes.data for o in outs for f in fields])
        check(self._lib.gsx_debug_render_pre(self.h, nv, cams, int(width), int(height), 1 if multi else 0, 1 if compact else 0, ptrs),
              self.h)
        for o in outs:
            o["dropped"] = int(o["dropped"][0])
        return outs

    def export_splat(self, path):
        """Write the uploaded splats as a `.splat` file: the viewer's 32-byte rows (position f32x3, exp(scale)
        f32x3, rgba u8x4, quaternion u8x4; gs.js:237, 539-542) in importance order.  The reference viewer takes
        such a file by drag and drop without re-parsing a 250-byte-per-vertex PLY in JavaScript."""
        buf, _, _ = self.render_debug()
        with open(path, "wb") as f:
            f.write(buf.tobytes())
        return len(buf)

    def sort_pairs(self, keys, values, bits=32):
        """Stable GPU radix sort by key bits [0, bits) (test hook, gsx_debug_sort_pairs)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(values, dtype=np.uint32).copy()
        check(self._lib.gsx_debug_sort_pairs(self.h, k.ctypes.data, v.ctypes.data, len(k), bits), self.h)
        return k, v

    def sort_pairs_drop(self, keys, values, bits=16):
        """The rasterizer's level-1 sort: pairs with key 0xffffffff are left out by the first pass; returns the kept pairs, sorted
        (stable) by key bits [0, bits) (test hook, gsx_debug_sort_pairs_drop)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(values, dtype=np.uint32).copy()
        kept = C.c_int64()
        check(self._lib.gsx_debug_sort_pairs_drop(self.h, k.ctypes.data, v.ctypes.data, len(k), bits, C.byref(kept)), self.h)
        return k[:kept.value], v[:kept.value]

    def sort_pairs_dev(self, keys, values, count, bits=32):
        """radix_sort_pairs_dev: len(keys) is the buffers' capacity, `count` is read on the device.  Returns (keys, values,
        where): the whole result buffer and which buffer pair it was (test hook, gsx_debug_sort_pairs_dev)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(values, dtype=np.uint32).copy()
        where = C.c_int32(-1)
        check(self._lib.gsx_debug_sort_pairs_dev(self.h, k.ctypes.data, v.ctypes.data, len(k), int(count), bits, C.byref(where)), self.h)
        return k, v, where.value

    def sort_values_wide(self, keys, values, count, bits, nranges):
        """The rasterizer's one-pass pair sort: (values (capacity,) u32 in the stable order of key bits [0, bits), ranges
        (nranges, 2) int32) (test hook, gsx_debug_sort_values_wide)."""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        v = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.empty(len(k), np.uint32)
        ranges = np.empty((int(nranges), 2), np.int32)
        check(self._lib.gsx_debug_sort_values_wide(self.h, k.ctypes.data, v.ctypes.data, len(k), int(count), bits, int(nranges),
                                                   out.ctypes.data, ranges.ctypes.data), self.h)
        return out, ranges

    def exclusive_scan(self, values):
        """(offsets (n,) u32, grand total as a Python int) of the rasterizer's scan (test hook, gsx_debug_exclusive_scan)."""
        a = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.empty(len(a), np.uint32)
        grand = C.c_uint64(0)
        check(self._lib.gsx_debug_exclusive_scan(self.h, a.ctypes.data, len(a), out.ctypes.data, C.byref(grand)), self.h)
        return out, int(grand.value)

    def ranges(self, sorted_keys, total, nlists):
        """(nlists, 2) int32 ranges of the sorted keys' first `total` entries (test hook, gsx_debug_ranges)."""
        k = np.ascontiguousarray(sorted_keys, dtype=np.uint32)
        out = np.empty((int(nlists), 2), np.int32)
        check(self._lib.gsx_debug_ranges(self.h, k.ctypes.data, len(k), int(total), int(nlists), out.ctypes.data), self.h)
        return out

    def debug_bin(self, tile_rect, rec, by_depth, nvis, div0, div1, m_cap, H, tiles_x, tiles_y, bin32=False, exact=False, sat=None,
                  pair_cap=1):
        """One depth phase's binning as a frame runs it, on the caller's arrays alone (test hook, gsx_debug_bin): tile_rect (n,) u32,
        rec (n,12) f32 or None, by_depth (len,) u32, sat None or u8 -> (count (m_cap,) u32, pair total as a Python int, keys
        (pair_cap,) u32, vals (pair_cap,) u32); what the kernels did not write is 0xFF bytes."""
        rect = np.ascontiguousarray(tile_rect, dtype=np.uint32)
        order = np.ascontiguousarray(by_depth, dtype=np.uint32)
        r = None if rec is None else np.ascontiguousarray(rec, dtype=np.float32)
        s = None if sat is None else np.ascontiguousarray(sat, dtype=np.uint8)
        lists = ((tiles_x + 1) // 2) * ((tiles_y + 1) // 2) * 4 if bin32 else tiles_x * tiles_y
        if (r is not None and r.size != 12 * len(rect)) or (s is not None and s.size != lists):
            raise ValueError("debug_bin: rec must hold 12 floats per splat, sat one byte per tile (bin32: four per bin)")
        count = np.empty(max(int(m_cap), 0), np.uint32)
        keys = np.empty(max(int(pair_cap), 0), np.uint32)
        vals = np.empty(max(int(pair_cap), 0), np.uint32)
        total = C.c_uint64(0)
        check(self._lib.gsx_debug_bin(self.h, len(rect), rect.ctypes.data, None if r is None else r.ctypes.data, order.ctypes.data,
                                      len(order), int(nvis), int(div0), int(div1), int(m_cap), int(H), int(tiles_x), int(tiles_y),
                                      1 if bin32 else 0, 1 if exact else 0, None if s is None else s.ctypes.data, int(pair_cap),
                                      count.ctypes.data, C.byref(total), keys.ctypes.data, vals.ctypes.data), self.h)
        return count, int(total.value), keys, vals

    def spatial_order(self):
        """The Morton order of the last upload_positions: perm[i] = uploaded index of slot i (test hook, gsx_debug_spatial_order)."""
        perm = np.empty(int(self._lib.gsx_num_gaussians(self.h)), np.uint32)
        check(self._lib.gsx_debug_spatial_order(self.h, perm.ctypes.data), self.h)
        return perm

    # -- IoU evaluation (Image_Segmentation/evaluation.py; csrc/iou.hip, csrc/iou_host.cpp) -------------------------------------
    def _iou_call(self, host_fn, dev_fn, lists, rest):
        """lists: [(device, items, dtype), ...] of one kind (all host or all device); rest(ptr arrays and dtypes) -> arguments"""
        device = lists[0][0]
        arrs = [(C.c_void_p * len(items))(*[t.data_ptr() if device else t.ctypes.data for t in items]) for _, items, _ in lists]
        if device:   # ONE fence for the whole call: the ctx stream is not torch's, and the call waits for its own results anyway
            import torch
            torch.cuda.current_stream().synchronize()
        check((dev_fn if device else host_fn)(self.h, *rest(arrs)), self.h)

    def iou_masks(self, masks, ground_truths):
        """IoU (evaluation.py:24-35) of every mask with every ground truth.  masks / ground_truths: lists of 2-D arrays (numpy, or
        torch tensors on this GPU) or one 3-D array each; a pixel is set iff value != 0.  Inputs are not written.
        Returns (iou float64 (M, G), inter int64 (M, G), area_masks int64 (M,), area_gt int64 (G,)); iou is NaN where both are empty."""
        m, g = _iou_same_side(_iou_list(masks, "masks"), _iou_list(ground_truths, "ground_truths"))
        (h, w), M, G = _iou_shape(m[1] + g[1]), len(m[1]), len(g[1])
        iou, inter = np.empty((M, G), np.float64), np.empty((M, G), np.int64)
        am, ag = np.empty(M, np.int64), np.empty(G, np.int64)
        self._iou_call(self._lib.gsx_iou_masks, self._lib.gsx_iou_masks_device, [m, g],
                       lambda a: (M, a[0], m[2], G, a[1], g[2], h, w, inter.ctypes.data, am.ctypes.data, ag.ctypes.data, iou.ctypes.data))
        return iou, inter, am, ag

    def best_ious(self, masks, ground_truths):
        """get_ious_from_masks (evaluation.py:38-56): [(max_iou, gt_idx), ...], one per mask; (0, 0) for a mask without a positive IoU."""
        best, idx = iou_best(self.iou_masks(masks, ground_truths)[0])
        return [(0, 0) if b == 0 else (b, int(i)) for b, i in zip(best, idx)]

    def label_map_tables(self, preds, gts, n_pred_classes, n_gt_classes, packed_u8=False):
        """Contingency tables of pairs of label maps (labels -1 .. n-1; any integer dtype; numpy or torch tensors on this GPU):
        int64 (n_pairs, P + 1, G + 1), entry [a, b] = pixels with pred label a - 1 and gt label b - 1.  packed_u8: uint8 maps hold
        label + 1.  A label out of range raises ValueError naming the pair and the lowest flat pixel index."""
        p, g = _iou_same_side(_iou_list(preds, "preds", seg=True, packed_u8=packed_u8), _iou_list(gts, "gts", seg=True, packed_u8=packed_u8))
        if len(p[1]) != len(g[1]):
            raise ValueError(f"label_map_tables: {len(p[1])} preds for {len(g[1])} gts")
        (h, w), n = _iou_shape(p[1] + g[1]), len(p[1])
        P, G = int(n_pred_classes), int(n_gt_classes)
        table = np.empty((n, max(P, 0) + 1, max(G, 0) + 1), np.int64)
        self._iou_call(self._lib.gsx_iou_label_maps, self._lib.gsx_iou_label_maps_device, [p, g],
                       lambda a: (n, a[0], p[2], P, a[1], g[2], G, h, w, table.ctypes.data))
        return table

    def masks_top_index(self, masks):
        """int32 (H, W): the highest list index whose mask is set at the pixel, or -1 - who owns the pixel in
        generate_segmentation_map (evaluation.py:65-67)."""
        m = _iou_list(masks, "masks", to_host=True)
        h, w = _iou_shape(m[1])
        out = np.empty((h, w), np.int32)
        self._iou_call(self._lib.gsx_masks_top_index, None, [m], lambda a: (len(m[1]), a[0], m[2], h, w, out.ctypes.data))
        return out

    # -- class maps from network outputs (deep_learning_segmentation.py:85-124, 142-144; csrc/segmap.hip) ---------------------------
    _FLOAT_DT = {"torch.float32": _lib.GSX_F32, "torch.float16": _lib.GSX_F16, "torch.bfloat16": _lib.GSX_BF16}

    def _seg_enter(self):
        """The ctx stream waits, on the device, for an event on torch's current stream - the producer of the inputs.
        Returns (ctx stream as torch's, torch's current stream); the caller lets the latter wait for the former once its kernels
        are queued, which also keeps torch's allocator honest: it hands a freed block only to work on the stream it was
        allocated on, and that stream is then behind the kernels that read or wrote the block.  (No Tensor.record_stream: it
        would leave the allocator with events to record on the ctx stream when a tensor dies - after close(), on a stream
        that no longer exists.)"""
        import torch
        dev = torch.device("cuda", self.device)
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(self.stream, device=dev)
        cur = torch.cuda.current_stream(dev)
        self._ext.wait_stream(cur)
        return self._ext, cur

    def order_after_torch(self):
        """The ctx stream waits, on the device, for torch's current stream: call it before vote_view on a tensor some torch
        operation has just written.  (segmap_from_logits / segmap_from_masks do it themselves; their results need none.)"""
        self._seg_enter()

    def _seg_input(self, t, what, dims):
        if not hasattr(t, "data_ptr") or not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what} must be a torch tensor on GPU {self.device}")
        if t.dim() not in dims:
            raise ValueError(f"{what} must have {' or '.join(str(d) for d in dims)} dimensions (got {tuple(t.shape)})")
        dt = self._FLOAT_DT.get(str(t.dtype))
        if dt is None:
            raise ValueError(f"{what} must be float32, float16 or bfloat16 (got {t.dtype})")
        return t.contiguous(), dt

    def segmap_from_logits(self, logits, size):
        """int32 class map(s) at the image size from a network's logits, on the device: logits (C, h, w) -> (height, width),
        (n, C, h, w) -> (n, height, width); size = (width, height).  torch.argmax over the channels, then OpenCV's nearest
        resize (deep_learning_segmentation.py:142-144).  Nothing is synchronised; the result goes straight into vote_view /
        vote_views_device, and torch's current stream is ordered behind it."""
        import torch
        t, dt = self._seg_input(logits, "logits", (3, 4))
        n, ch, h, w = (1,) + tuple(t.shape) if t.dim() == 3 else tuple(t.shape)
        W, H = int(size[0]), int(size[1])
        if W <= 0 or H <= 0:
            raise ValueError(f"size must be positive (got {W} x {H})")
        out = torch.empty((H, W) if t.dim() == 3 else (n, H, W), dtype=torch.int32, device=t.device)
        ext, cur = self._seg_enter()
        check(self._lib.gsx_segmap_from_logits(self.h, t.data_ptr(), dt, n, ch, h, w, W, H, out.data_ptr()), self.h)
        cur.wait_stream(ext)
        return out

    def segmap_from_masks(self, masks, cls, conf, size):
        """int32 (height, width) class map from instance masks (K, mh, mw), class ids (K,) and confidences (K,), all on the
        device: the loop of process_yolo_segmentation (deep_learning_segmentation.py:113-124).  -1 where no accepted instance
        (conf > 0.5) has a mask value > 0.5; later instances overwrite earlier ones.  masks may be None or empty (K = 0).
        conf is never read on the host: nothing is synchronised."""
        import torch
        W, H = int(size[0]), int(size[1])
        if W <= 0 or H <= 0:
            raise ValueError(f"size must be positive (got {W} x {H})")
        dev = torch.device("cuda", self.device)
        K = 0 if masks is None else int(masks.shape[0])
        if K == 0:
            mh, mw = (1, 1) if masks is None or masks.dim() != 3 or 0 in masks.shape[1:] else (int(masks.shape[1]), int(masks.shape[2]))
            out = torch.empty((H, W), dtype=torch.int32, device=dev)
            ext, cur = self._seg_enter()
            check(self._lib.gsx_segmap_from_masks(self.h, None, _lib.GSX_F32, 0, mh, mw, None, None, W, H, out.data_ptr()), self.h)
            cur.wait_stream(ext)
            return out
        t, dt = self._seg_input(masks, "masks", (3,))
        mh, mw = int(t.shape[1]), int(t.shape[2])
        cc = [torch.as_tensor(v, device=dev).to(torch.float32).reshape(-1).contiguous() for v in (cls, conf)]
        if any(v.numel() != K for v in cc):
            raise ValueError(f"cls and conf must hold one value per mask ({K})")
        out = torch.empty((H, W), dtype=torch.int32, device=dev)
        ext, cur = self._seg_enter()
        check(self._lib.gsx_segmap_from_masks(self.h, t.data_ptr(), dt, K, mh, mw, cc[0].data_ptr(), cc[1].data_ptr(), W, H, out.data_ptr()),
              self.h)
        cur.wait_stream(ext)
        return out

    def segmap_from_queries(self, masks, slot_query, slot_score, size, slot_label=None, mid=(384, 384), threshold=0.5, labels=False,
                            return_slots=False):
        """int32 (height, width) map from Mask2Former's query outputs, on the device: what transformers'
        post_process_instance_segmentation(outputs, target_sizes=[(height, width)]) does after its softmax / top-k
        (deep_learning_segmentation.py:156-158).  masks (Q, h, w) mask logits; slot_query, slot_score, slot_label (K,): query
        index, score and class of the selected slots, in the selection's order (select_query_slots); size and mid = (width,
        height).  The map holds segment ids 0, 1, .. in acceptance order and -1 for the background, as the reference's does;
        labels=True writes each segment's slot_label instead.  return_slots: also (slot_segment int32 (K,), slot_pred float32
        (K,)), the segment id (-1: rejected) and the score of every slot - segments_info, on the device.  Nothing is
        synchronised."""
        import torch
        W, H = int(size[0]), int(size[1])
        mid_w, mid_h = int(mid[0]), int(mid[1])
        if min(W, H, mid_w, mid_h) <= 0:
            raise ValueError(f"size and mid must be positive (got {W} x {H}, {mid_w} x {mid_h})")
        t, dt = self._seg_input(masks, "masks", (3,))
        Q, h, w = (int(v) for v in t.shape)
        dev = t.device
        sq = torch.as_tensor(slot_query, device=dev).to(torch.int32).reshape(-1).contiguous()
        ss = torch.as_tensor(slot_score, device=dev).to(torch.float32).reshape(-1).contiguous()
        K = int(sq.numel())
        if labels and slot_label is None:
            raise ValueError("labels=True needs slot_label")
        sl = None if slot_label is None else torch.as_tensor(slot_label, device=dev).to(torch.int32).reshape(-1).contiguous()
        if ss.numel() != K or (sl is not None and sl.numel() != K):
            raise ValueError(f"slot_query, slot_score and slot_label must hold one value per slot ({K})")
        out = torch.empty((H, W), dtype=torch.int32, device=dev)
        seg = torch.empty(K, dtype=torch.int32, device=dev) if return_slots else None
        pred = torch.empty(K, dtype=torch.float32, device=dev) if return_slots else None
        ptr = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
        ext, cur = self._seg_enter()
        check(self._lib.gsx_segmap_from_queries(self.h, t.data_ptr(), dt, Q, h, w, K, ptr(sq), ptr(ss), ptr(sl), mid_w, mid_h, float(threshold),
                                                _lib.GSX_QUERIES_LABELS if labels else _lib.GSX_QUERIES_SEGMENTS, W, H, out.data_ptr(),
                                                ptr(seg), ptr(pred)), self.h)
        cur.wait_stream(ext)
        return (out, seg, pred) if return_slots else out

    def synchronize(self):
        check(self._lib.gsx_synchronize(self.h), self.h)
        self._keep_alive.clear()

    @property
    def stream(self):
        return self._lib.gsx_stream(self.h)

    # -- profiling ---------------------------------------------------------------------------------
    def profile(self, on=True):
        check(self._lib.gsx_profile_enable(self.h, 1 if on else 0), self.h)
        check(self._lib.gsx_profile_reset(self.h), self.h)

    def profile_names(self):
        out, i = [], 0
        while True:
            nm = self._lib.gsx_profile_name(self.h, i)
            if nm is None:
                return out
            out.append(nm.decode())
            i += 1

    def profile_get(self, name):
        n, ms = C.c_int64(), C.c_double()
        check(self._lib.gsx_profile_get(self.h, name.encode(), C.byref(n), C.byref(ms)), self.h)
        return n.value, ms.value


def bind_to_gpu_numa_node(device=0):
    """One process per GPU: keep this process (and every thread it starts from now on) on the CPUs of the NUMA node the
    GPU hangs off (/sys/bus/pci/devices/<bdf>/local_cpulist), so that the segmentation maps it allocates, the pinned
    staging ring and the packer threads all sit next to the GPU's PCIe root.  Returns the CPU set, or None when the
    kernel does not expose the topology or the process may not run there (then nothing is changed)."""
    try:
        import torch
        p = torch.cuda.get_device_properties(device)
        bdf = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
        txt = open(f"/sys/bus/pci/devices/{bdf}/local_cpulist").read().strip()
        cpus = set()
        for part in txt.split(","):
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus or cpus == os.sched_getaffinity(0):
            return None
        os.sched_setaffinity(0, cpus)
        return cpus
    except Exception:
        return None


def cull_planes(camera):
    """The five world-space culling planes of one view (test hook, host only): array (5, 5) = unit normal A, offset B,
    margin slope M; a sphere (c, r) is skipped when A.c + B > r + M * (|c|_1 + r) for one of them."""
    cam = camera if isinstance(camera, Camera) else Camera.from_dict(camera)
    out = np.empty((5, 5), np.float64)
    check(_lib.lib().gsx_debug_cull_planes(C.byref(cam), out.ctypes.data))
    return out


def project_gaussian(position, camera, ctx=None):
    """Device-side project_gaussian (reference :43-82): (x, y) ints or None."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        return ctx.project_one(position, camera)
    finally:
        if own:
            ctx.close()


def assign_labels_from_maps(gaussians, cameras, segmaps, image_sizes=None, n_classes=150, ctx=None):
    """Majority vote given per-camera segmentation maps.

    cameras / segmaps / image_sizes are parallel lists over the cameras that the reference would
    actually process (missing images already skipped, deep_learning_segmentation.py:256-259).
    Returns int32 labels (N,), bit-identical to the reference's assign_labels (:297-308)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.upload_positions(gaussians)
        ctx.vote_begin(n_classes, 0, max(1, len(cameras)))
        for k, (cam, seg) in enumerate(zip(cameras, segmaps)):
            ctx.vote_view(cam, seg, None if image_sizes is None else image_sizes[k])
        return ctx.vote_finalize()
    finally:
        if own:
            ctx.close()


def assign_instances_from_maps(gaussians, cameras, segmaps, image_sizes=None, max_instances=255, min_overlap=0.3, min_size=1, ctx=None):
    """Instance labels from per-view SEGMENT maps (ids numbered per image, -1 .. 253; Mask2Former's default map): every map is
    first associated with the instances the Gaussians already carry (Context.assoc_view), then the relabelled maps are voted
    like class maps.  Arguments as assign_labels_from_maps.  Returns (int32 labels (N,), number of instances)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.upload_positions(gaussians)
        ctx.assoc_begin(254, max_instances, min_overlap, min_size)
        ctx.vote_begin(max_instances, 0, max(1, len(cameras)))
        for k, (cam, seg) in enumerate(zip(cameras, segmaps)):
            size = None if image_sizes is None else image_sizes[k]
            ctx.vote_view(cam, ctx.assoc_view(cam, seg, size)[1], size)
        return ctx.vote_finalize(), ctx.assoc_num_instances()
    finally:
        if own:
            ctx.close()


def label_maps_from_labels(splats, labels, cameras, sizes, n_classes, min_weight=0.0, ctx=None):
    """The class maps a labelled scene shows: splats = (xyz, scale, rot, opacity, f_dc) as for Context.upload_splats, labels
    int (N,) in [-1, n_classes - 1], cameras / sizes parallel lists of cameras.json dicts and (width, height) of the wanted
    maps (the camera's fx, fy are scaled to that size).  The frames use the viewer's camera convention, as lift_view does.
    Returns a list of int32 (height, width) maps (Context.label_view)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.upload_splats(*splats, labels=labels)
        return [ctx.label_view(cam, int(size[0]), int(size[1]), n_classes, min_weight) for cam, size in zip(cameras, sizes)]
    finally:
        if own:
            ctx.close()


def depth_maps(splats, cameras, sizes, quantile=0.5, ctx=None):
    """The depth frames of a scene: splats = (xyz, scale, rot, opacity, f_dc) as for Context.upload_splats, cameras / sizes
    parallel lists of cameras.json dicts and (width, height) of the wanted maps (the camera's fx, fy are scaled to that size).
    The frames use the viewer's camera convention.  Returns a list of DepthFrame (Context.depth_view)."""
    own = ctx is None
    ctx = ctx or Context()
    try:
        ctx.upload_splats(*splats)
        return [ctx.depth_view(cam, int(size[0]), int(size[1]), quantile) for cam, size in zip(cameras, sizes)]
    finally:
        if own:
            ctx.close()


def host_pack(seg_map, n_classes, tiled=True, coarse=True, threads=1, packed_u8=False):
    """Test hook, no GPU: the packed form gsx_vote_view stages for a host map -> (bytes u8, coarse_off or -1, bad)."""
    seg = np.asarray(seg_map)
    if seg.dtype == np.int64:
        dt = _lib.GSX_SEG_I64
    elif seg.dtype == np.uint8:
        dt = _lib.GSX_SEG_U8 if packed_u8 else _lib.GSX_SEG_U8_LABELS
    else:
        seg, dt = seg.astype(np.int32, copy=False), _lib.GSX_SEG_I32
    seg = np.ascontiguousarray(seg)
    h, w = seg.shape
    nbytes, coff, bad = C.c_int64(), C.c_int64(), C.c_int32()
    L = _lib.lib()
    check(L.gsx_debug_host_pack(seg.ctypes.data, dt, w, h, n_classes, int(tiled), int(coarse), threads, None, 0, C.byref(nbytes),
                                C.byref(coff), C.byref(bad)))
    out = np.zeros(nbytes.value, np.uint8)
    check(L.gsx_debug_host_pack(seg.ctypes.data, dt, w, h, n_classes, int(tiled), int(coarse), threads, out.ctypes.data, out.size,
                                C.byref(nbytes), C.byref(coff), C.byref(bad)))
    return out, coff.value, bool(bad.value)


def region_grow(normals, residuals, knn, residual_threshold=0.1, angle_threshold=0.05):
    """segmentation_3D (3D_clustering/region_growing.py:166-226) on the host, no context: normals (n, 3), residuals (n,),
    knn (n, k) neighbour lists in visiting order.  Returns (labels int32 (n,), n_regions); label 0 is the largest region."""
    nrm = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    res = np.ascontiguousarray(residuals, np.float64).reshape(-1)
    nb = np.ascontiguousarray(knn, np.int32)
    if nb.ndim != 2 or len(nb) != len(nrm) or len(res) != len(nrm):
        raise ValueError("normals (n, 3), residuals (n,) and knn (n, k) must agree in n")
    labels = np.empty(len(nrm), np.int32)
    nreg = C.c_int32(0)
    check(_lib.lib().gsx_region_grow(len(nrm), nrm.ctypes.data, res.ctypes.data, nb.ctypes.data, nb.shape[1], float(residual_threshold),
                                     float(angle_threshold), labels.ctypes.data, C.byref(nreg)))
    return labels, int(nreg.value)


def debug_nn_grid(points, k, brute=False):
    """Test hook, no context and no GPU: the search grid gsx_normals / gsx_knn build for these points and this k.
    Returns (origin float64 (3,), cell edge h, dims int32 (3,), cell_start uint32 (cells + 1,), order int32 (n,): the
    original index at each position of the cell-sorted points; cells are numbered x fastest)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    origin, h, dims = np.empty(3, np.float64), C.c_double(), np.empty(3, np.int32)
    L = _lib.lib()
    check(L.gsx_debug_nn_grid(len(pts), pts.ctypes.data, int(k), int(bool(brute)), origin.ctypes.data, C.byref(h), dims.ctypes.data, None, None))
    start = np.empty(int(np.prod(dims.astype(np.int64))) + 1, np.uint32)
    order = np.empty(len(pts), np.int32)
    check(L.gsx_debug_nn_grid(len(pts), pts.ctypes.data, int(k), int(bool(brute)), origin.ctypes.data, C.byref(h), dims.ctypes.data,
                              start.ctypes.data, order.ctypes.data))
    return origin, float(h.value), dims, start, order


# -- IoU evaluation: input normalisation and the host-only helpers --------------------------------------------------------------------
_MASK_NP = {"u1": _lib.GSX_MASK_U8, "i4": _lib.GSX_MASK_I32, "i8": _lib.GSX_MASK_I64, "f4": _lib.GSX_MASK_F32, "f8": _lib.GSX_MASK_F64}
_MASK_NP_AS = {"b1": ("view", np.uint8), "i1": ("view", np.uint8), "i2": ("to", np.int32), "u2": ("to", np.int32), "u4": ("view", np.int32),
               "u8": ("view", np.int64), "f2": ("to", np.float32)}   # same width: the bits decide "!= 0"; narrower: widened exactly


def _iou_mask_np(a):
    a = np.ascontiguousarray(a)
    key = a.dtype.str[1:] if a.dtype.kind in "buif" else ""
    how = _MASK_NP_AS.get(key)
    if how:
        a = a.view(how[1]) if how[0] == "view" else a.astype(how[1])
    elif key not in _MASK_NP:
        a = (a != 0).view(np.uint8)
    return a, _MASK_NP[a.dtype.str[1:]]


def _iou_mask_torch(t):
    import torch
    t = t.contiguous()
    if t.dtype in (torch.bool, torch.int8):
        t = t.view(torch.uint8)
    elif t.dtype == torch.int16:
        t = t.to(torch.int32)
    elif t.dtype in (torch.float16, torch.bfloat16):
        t = t.to(torch.float32)
    code = {torch.uint8: _lib.GSX_MASK_U8, torch.int32: _lib.GSX_MASK_I32, torch.int64: _lib.GSX_MASK_I64,
            torch.float32: _lib.GSX_MASK_F32, torch.float64: _lib.GSX_MASK_F64}.get(t.dtype)
    if code is None:
        t, code = (t != 0).view(torch.uint8), _lib.GSX_MASK_U8
    return t, code


def _iou_list(x, what, seg=False, packed_u8=False, to_host=False):
    """-> (device, [2-D contiguous arrays or tensors of ONE supported dtype], dtype code)"""
    if hasattr(x, "data_ptr") or isinstance(x, np.ndarray):
        if x.ndim not in (2, 3):
            raise ValueError(f"{what}: expected a list of 2-D arrays or one 3-D array")
        x = [x] if x.ndim == 2 else list(x)
    x = list(x)
    if not x:
        raise ValueError(f"{what}: empty list")
    device = all(hasattr(t, "data_ptr") and t.is_cuda for t in x) and not to_host
    if not device:
        x = [t.detach().cpu().numpy() if hasattr(t, "data_ptr") else np.asarray(t) for t in x]
    if any(t.ndim != 2 for t in x):
        raise ValueError(f"{what}: every entry must be 2-D")
    if seg:
        out, codes = [], []
        for t in x:
            t, code = _seg_map_arg(t, packed_u8)[:2]
            out.append(t)
            codes.append(code)
        if len(set(codes)) > 1:   # mixed dtypes: int64 holds them all (a packed uint8 map is unpacked on the way)
            wide = [t.long() if device else t.astype(np.int64) for t in out]
            out = [t - 1 if c == _lib.GSX_SEG_U8 else t for t, c in zip(wide, codes)]
            codes = [_lib.GSX_SEG_I64]
        return device, out, codes[0]
    pairs = [(_iou_mask_torch if device else _iou_mask_np)(t) for t in x]
    if len({c for _, c in pairs}) > 1:   # mixed dtypes: every non-zero value stays non-zero as a double, and -0.0 stays -0.0
        pairs = [((t.double() if device else t.astype(np.float64)), _lib.GSX_MASK_F64) for t, _ in pairs]
    return device, [t for t, _ in pairs], pairs[0][1]


def _iou_same_side(a, b):
    """both lists on the host or both on the device: a device list next to a host list comes down"""
    if a[0] == b[0]:
        return a, b
    down = lambda l: (False, [np.ascontiguousarray(t.cpu().numpy()) for t in l[1]], l[2]) if l[0] else l
    return down(a), down(b)


def _iou_shape(items):
    shape = tuple(items[0].shape)
    for t in items:
        if tuple(t.shape) != shape:
            raise ValueError(f"all masks / maps of a call must share one shape: {tuple(t.shape)} next to {shape}")
    return shape


def iou_from_counts(inter, area_a, area_b):
    """inter / (area_a + area_b - inter) as the reference divides (evaluation.py:35), elementwise over int64 arrays of one
    shape; NaN where the union is empty.  Host only."""
    inter = np.ascontiguousarray(inter, np.int64)
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(area_a, np.int64), inter.shape))
    b = np.ascontiguousarray(np.broadcast_to(np.asarray(area_b, np.int64), inter.shape))
    out = np.empty(inter.shape, np.float64)
    check(_lib.lib().gsx_iou_from_counts(inter.size, inter.ctypes.data, a.ctypes.data, b.ctypes.data, out.ctypes.data))
    return out


def iou_from_table(table):
    """float64 (..., P + 1, G + 1) from contingency tables: entry [a, b] = n_ab / (row_a + col_b - n_ab), which is exactly
    IoU(pred == a - 1, gt == b - 1) of the reference (evaluation.py:24-35); NaN where neither label occurs.  Host only."""
    t = np.asarray(table, np.int64)
    if t.ndim < 2:
        raise ValueError("iou_from_table: a table has at least two axes")
    return iou_from_counts(t, t.sum(axis=-1, keepdims=True), t.sum(axis=-2, keepdims=True))


def iou_best(iou):
    """The best match of get_ious_from_masks (evaluation.py:44-54) over iou (M, G): (best float64 (M,), gt_idx int32 (M,)).
    Strict '>' from (0, gt 0): the first of equal maxima wins, NaN never wins, no positive IoU gives (0, 0).  Host only."""
    iou = np.ascontiguousarray(iou, np.float64)
    if iou.ndim != 2:
        raise ValueError("iou_best: iou must be 2-D (masks, ground truths)")
    best, idx = np.empty(iou.shape[0], np.float64), np.empty(iou.shape[0], np.int32)
    check(_lib.lib().gsx_iou_best(iou.shape[0], iou.shape[1], iou.ctypes.data, best.ctypes.data, idx.ctypes.data))
    return best, idx


def segmap_constants():
    """Test hook, host only: the units the class-map kernels are built on (gsx_debug_segmap_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_segmap_constants(out.ctypes.data))
    return {"pix_wg": int(out[0]), "slices": int(out[1]), "step": int(out[2]), "vec": int(out[3]), "resize_vec": int(out[4]),
            "resize_block": int(out[5]), "block": int(out[6])}


def queries_constants():
    """Test hook, host only: the units the Mask2Former query kernels are built on (gsx_debug_queries_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_queries_constants(out.ctypes.data))
    names = ("cols", "rows_wg", "rows_wave", "scan_word", "accept_waves", "max_slots", "block")
    return dict(zip(names, (int(v) for v in out)))


def segpack_constants():
    """Test hook, host only: the units the device map pack and the host map hand-over are built on (gsx_debug_segpack_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_segpack_constants(out.ctypes.data))
    names = ("block", "batch", "strip_cols", "band_rows", "cstrip_cells", "cband_rows", "dma_batch", "compact_batch")
    return dict(zip(names, (int(v) for v in out)))


def iou_constants():
    """Test hook, host only: the units the IoU kernels are built on (gsx_debug_iou_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_iou_constants(out.ctypes.data))
    names = ("load_bytes", "word_bits", "wave_tile", "block_tile", "pair_tile", "pair_chunk_words", "table_lds_max", "table_run")
    return dict(zip(names, (int(v) for v in out)))


def assoc_constants():
    """Test hook, host only: the units the association kernels are built on (gsx_debug_assoc_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_assoc_constants(out.ctypes.data))
    names = ("one", "shift", "block", "max_segments", "max_instances", "lds_entries", "max_chunks")
    return dict(zip(names, (int(v) for v in out)))


def smooth_constants():
    """Test hook, host only: the units the label filter's two forms are built on (gsx_debug_smooth_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_smooth_constants(out.ctypes.data))
    names = ("list_max_k", "max_classes", "counter_bits", "lanes", "waves")
    return dict(zip(names, (int(v) for v in out)))


def labelmap_constants():
    """Test hook, host only: the units the label-frame kernel is built on (gsx_debug_labelmap_constants); window = WL, the
    labels a tile accumulates per walk of its list."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_labelmap_constants(out.ctypes.data))
    names = ("one", "shift", "tile", "chunk", "window", "max_classes")
    return dict(zip(names, (int(v) for v in out)))


def depth_constants():
    """Test hook, host only: the units the depth-frame kernel is built on (gsx_debug_depth_constants)."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_depth_constants(out.ctypes.data))
    names = ("one", "shift", "tile", "chunk")
    return dict(zip(names, (int(v) for v in out)))


def lift_constants():
    """Test hook, host only: the units the lifting kernel is built on (gsx_debug_lift_constants); one = GSX_LIFT_ONE."""
    out = np.zeros(8, np.int32)
    check(_lib.lib().gsx_debug_lift_constants(out.ctypes.data))
    names = ("one", "shift", "tile", "chunk", "cells", "loop_max", "max_classes")
    return dict(zip(names, (int(v) for v in out)))
