"""Thin Python object over a ``dsir_ctx`` (include/dsir.h).

PyTorch is used for device memory only: every method takes / returns
``torch`` CUDA tensors and hands raw device pointers to the C ABI.  All
compute is in libdsir.so; nothing here falls back to torch ops or the CPU.

Activations crossing this boundary are point-major ``[clouds, n, C]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .arch import PIPELINES, NetConfig, level_sizes


class EngineError(RuntimeError):
    pass


def check_pose_weight(w) -> float:
    """wt_pose_loss as the loss entries take it: finite and >= 0 (dsir_align_loss_backward3 rejects anything else, too)."""
    w = float(w)
    if not (w >= 0.0) or w == float("inf"):
        raise EngineError(f"align_loss_backward: wt_pose_loss must be finite and >= 0, got {w}")
    return w


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise EngineError(f"{name}: expected a CUDA tensor (the engine has no CPU path)")
    if t.dtype != dtype:
        raise EngineError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def pair_counts(counts, P: int, cap: int, name: str):
    """Per-pair row counts as the ICP entries take them (include/dsir.h, dsir_icp_refine_ex3): None, or [P] integers in
    [0, cap] as a sequence, an array or a tensor -> None, or the counts as a host int32 array.  ValueError for anything else:
    the C ABI would clamp a count, the host wrapper refuses it."""
    if counts is None:
        return None
    a = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if a.shape != (P,) or a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold {P} integers (one per pair), got shape {tuple(a.shape)} of {a.dtype}")
    if P and (int(a.min()) < 0 or int(a.max()) > cap):
        raise ValueError(f"{name} must lie in [0, {cap}] (the rows of the array), got {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a, np.int32)


ICP_KERNELS = {"l2": 0, "huber": 1, "cauchy": 2, "gm": 3, "tukey": 4}        # include/dsir.h DSIR_ICP_L2 .. DSIR_ICP_TUKEY


def icp_kernel_args(kernel, kernel_scale):
    """The robust-kernel arguments of the ICP entries (include/dsir.h, dsir_icp_refine_ex4): a name of ICP_KERNELS and, for a kernel
    other than "l2", a scale whose fp32 value is finite and positive -> (kernel number, fp32 scale as a float; 0.0 under "l2", whose
    scale is ignored).  ValueError for anything else."""
    if not isinstance(kernel, str) or kernel not in ICP_KERNELS:
        raise ValueError(f"kernel must be one of {', '.join(ICP_KERNELS)}, got {kernel!r}")
    if kernel == "l2":
        return 0, 0.0
    try:
        with np.errstate(over="ignore"):
            k = float(np.float32(kernel_scale))
    except (TypeError, ValueError):
        k = float("nan")
    if not (np.isfinite(k) and k > 0.0):
        raise ValueError(f"kernel_scale must be a finite positive number (as fp32) with kernel={kernel!r}, got {kernel_scale!r}")
    return ICP_KERNELS[kernel], k


class Engine:
    def __init__(self, cfg: NetConfig, device: int = 0, max_points: int = 8192, max_pairs: int = 1):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.max_points, self.max_pairs = int(max_points), int(max_pairs)
        c = _lib.dsir_cfg()
        c.feat_len, c.num_knn, c.num_layers = cfg.feat_len, cfg.num_knn, len(cfg.d_out)
        for i in range(4):
            c.sub_sampling_ratio[i] = cfg.sub_sampling_ratio[i]
            c.d_out[i] = cfg.d_out[i]
        c.out_feat_dim, c.num_classes = cfg.out_feat_dim, cfg.num_classes
        c.max_points, c.max_pairs = self.max_points, self.max_pairs
        c.pipeline = PIPELINES.index(cfg.pipeline)
        h = C.c_void_p()
        # use_ppf (reference RandLANet.py:251-254): feat_len is then the width of a point row, xyz + normal (+ ignored columns)
        flags = _lib.DSIR_FLAG_PPF if cfg.use_ppf else 0
        if self.lib.dsir_create_ex(device, C.byref(c), flags, C.byref(h)) != 0:
            raise EngineError("dsir_create: " + self.lib.dsir_last_error(None).decode())
        self.h = h
        self.weights_loaded = False
        self._shared_stream = False
        self._bound_stream = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.dsir_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _call(self, rc: int):
        if rc != 0:
            raise EngineError(self.lib.dsir_last_error(self.h).decode())

    def _pre(self):
        if not self._shared_stream:
            torch.cuda.current_stream(self.device).synchronize()
            return
        # shared mode follows torch's current stream (torch.cuda.graph captures on a side stream): re-bind when it changed
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if cur != self._bound_stream:
            self._call(self.lib.dsir_set_stream(self.h, C.c_void_p(cur), 0))
            self._bound_stream = cur

    def sync(self):
        if not self._shared_stream:     # on the caller's stream the results are stream-ordered with the caller's own kernels
            self._call(self.lib.dsir_sync(self.h))

    def use_torch_stream(self, on: bool = True):
        """Order the engine's operators on torch's CURRENT stream (include/dsir.h, dsir_set_stream) instead of the context's
        own: no host synchronisation around a call any more (results are stream-ordered with torch's kernels), which also makes
        the operators capturable by ``torch.cuda.graph``.  ``on=False``: back to the context's own stream (after a device
        synchronisation, so that nothing enqueued on torch's stream is overtaken)."""
        if on:
            self._call(self.lib.dsir_sync(self.h))
            self._bound_stream = torch.cuda.current_stream(self.device).cuda_stream
            self._call(self.lib.dsir_set_stream(self.h, C.c_void_p(self._bound_stream), 0))
            self._shared_stream = True
        else:
            torch.cuda.synchronize(self.device)
            self._call(self.lib.dsir_set_stream(self.h, None, 1))
            self._shared_stream = False
            self._bound_stream = None

    def _empty(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    # ------------------------------------------------------------------ weights
    def expected_keys(self):
        n = self.lib.dsir_num_weights(self.h)
        out = []
        for i in range(n):
            numel = C.c_int64()
            out.append((self.lib.dsir_weight_name(self.h, i, C.byref(numel)).decode(), numel.value))
        return out

    def load_state_dict(self, sd: Dict[str, "np.ndarray | torch.Tensor"], strict: bool = True):
        """Network.load_state_dict counterpart (reference test.py:614): strict key/shape checking."""
        expected = [k for k, _ in self.expected_keys()]
        missing = [k for k in expected if k not in sd]
        unexpected = [k for k in sd if k not in set(expected)]
        if strict and (missing or unexpected):
            raise EngineError(f"Error(s) in loading state_dict: missing keys {missing[:5]}{'...' if len(missing) > 5 else ''}, "
                              f"unexpected keys {unexpected[:5]}{'...' if len(unexpected) > 5 else ''}")
        for k in expected:
            if k not in sd:
                continue
            v = sd[k]
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if k.endswith("num_batches_tracked"):
                self._call(self.lib.dsir_load_weight(self.h, k.encode(), None, None, 0))
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._call(self.lib.dsir_load_weight(self.h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))
        self._call(self.lib.dsir_finalize_weights(self.h))
        self.weights_loaded = True

    # ------------------------------------------------------------------ stages
    def pyramid_shapes(self, n: int) -> Tuple[int, int]:
        nl = level_sizes(n, self.cfg.sub_sampling_ratio)
        return sum(nl[:-1]), sum(nl[1:])

    def narrow(self, t: torch.Tensor) -> torch.Tensor:
        """int64 index tensor -> int32 (on device)."""
        if t.dtype == torch.int32:
            return t.contiguous()
        t = _chk(t, torch.int64, "index tensor")
        out = self._empty(t.shape, torch.int32)
        self._pre()
        self._call(self.lib.dsir_narrow_i64(self.h, _ptr(t), _ptr(out), t.numel()))
        self.sync()                     # as every other stage: the result is ready for torch's stream when the call returns
        return out

    def knn_pyramid(self, points: torch.Tensor):
        """DataBase.nn_search counterpart.  points [clouds, n, >=3] ->
        (xyz [c,S,3], neigh_idx [c,S,16] i32, sub_idx [c,S1,16] i32, interp_idx [c,S,1] i32)."""
        points = _chk(points, torch.float32, "points")
        c, n, stride = points.shape
        S, S1 = self.pyramid_shapes(n)
        xyz = self._empty((c, S, 3))
        neigh = self._empty((c, S, 16), torch.int32)
        sub = self._empty((c, S1, 16), torch.int32)
        interp = self._empty((c, S, 1), torch.int32)
        self._pre()
        self._call(self.lib.dsir_knn_pyramid(self.h, _ptr(points), stride, c, n, _ptr(xyz), _ptr(neigh), _ptr(sub), _ptr(interp)))
        self.sync()
        return xyz, neigh, sub, interp

    def randla_forward(self, which: str, features, xyz, neigh, sub, interp, want_logits=True):
        """RandLA.forward counterpart -> (feat [c,n,64], logits [c,n,ncls])."""
        features = _chk(features, torch.float32, "features")
        c, n, cin = features.shape
        w = {"feat_extractor": 0, "inlier_model": 1}[which]
        ncls = self.cfg.num_classes if w == 0 else 1
        feat = self._empty((c, n, 64))
        logits = self._empty((c, n, ncls)) if want_logits else None
        xyz, neigh, sub, interp = (_chk(xyz, torch.float32, "xyz"), _chk(neigh, torch.int32, "neigh_idx"),
                                   _chk(sub, torch.int32, "sub_idx"), _chk(interp, torch.int32, "interp_idx"))
        self._pre()
        self._call(self.lib.dsir_randla_forward(self.h, w, _ptr(features), cin, c, n, _ptr(xyz), _ptr(neigh), _ptr(sub),
                                                _ptr(interp), _ptr(feat), _ptr(logits)))
        self.sync()
        return feat, logits

    def lfa_enc2_probe(self, which: str, level: int, fused: bool, xyz, neigh, n: int):
        """Debug entry (include/dsir.h, dsir_lfa_enc2_probe): lfa.mlp2 of one pyramid level alone, by the row-streaming launch
        (fused=False) or by the first pooling's producing variant (fused=True); xyz / neigh: the pyramid of clouds of n points ->
        (rows [c, 16 n_level, d/2] raw convolution
        outputs, stats [c, groups, 4] float64 as committed; groups as the engine assigns them: 8 from 64 channels up, else 4)."""
        xyz, neigh = _chk(xyz, torch.float32, "xyz"), _chk(neigh, torch.int32, "neigh_idx")
        c = xyz.shape[0]
        assert xyz.shape[1] == self.pyramid_shapes(n)[0]
        nl = n
        for r in self.cfg.sub_sampling_ratio[:level]:
            nl //= r
        ch = self.cfg.d_out[level] // 2
        rows = self._empty((c, 16 * nl, ch))
        stats = self._empty((c, 8 if ch >= 64 else 4, 4), torch.float64)
        self._pre()
        self._call(self.lib.dsir_lfa_enc2_probe(self.h, {"feat_extractor": 0, "inlier_model": 1}[which], level, int(fused), c, n, _ptr(xyz),
                                                _ptr(neigh), _ptr(rows), _ptr(stats)))
        self.sync()
        return rows, stats

    def mlp_feat_probe(self, feat0, fused: int, max_workgroups: int = 0):
        """Debug entry (include/dsir.h, dsir_mlp_feat_probe): mlp_feat alone, feat0 [c,n,64] -> [c,n,64], by the three point-wise
        launches (fused=0), the one fused launch (1), or the fused launch on both halves of the clouds with two output bases (2);
        max_workgroups > 0 caps the fused launch's grid (a wave then walks several row tiles)."""
        feat0 = _chk(feat0, torch.float32, "feat0")
        c, n, ch = feat0.shape
        assert ch == 64
        out = self._empty((c, n, 64))
        self._pre()
        self._call(self.lib.dsir_mlp_feat_probe(self.h, _ptr(feat0), c, n, int(fused), int(max_workgroups), _ptr(out)))
        self.sync()
        return out

    def ppf_pre(self, which: str, rows, neigh_multi):
        """The use_ppf front end of RandLA.forward (RandLANet.py:324-332; csrc/ppf.hip): rows [c,n,>=6] = xyz + normal,
        neigh_multi the pyramid's neigh_idx [c,S,16] (its level-0 rows are read) -> [c,n,12], the input of level 0."""
        rows, neigh_multi = _chk(rows, torch.float32, "rows"), _chk(neigh_multi, torch.int32, "neigh_idx")
        c, n, stride = rows.shape
        out = self._empty((c, n, 12))
        self._pre()
        self._call(self.lib.dsir_ppf_pre(self.h, {"feat_extractor": 0, "inlier_model": 1}[which], _ptr(rows), stride, _ptr(neigh_multi),
                                         neigh_multi.shape[1] * 16, c, n, _ptr(out)))
        self.sync()
        return out

    def estimate_normals(self, points, neigh_multi=None, viewpoint=(0.0, 0.0, 0.0), csr=None):
        """Normals from neighbour lists (include/dsir.h, dsir_estimate_normals / dsir_estimate_normals_csr; the rule: deepsir_amd/ppf.py):
        points [c,n,>=3] and exactly one of neigh_multi [c,S,16] (the pyramid's level-0 lists) and csr = (offsets [c n + 1] i32, cols
        i32 with cloud-local columns: what ``radius_neighbors`` returns; a row of fewer than 3 entries is degenerate) ->
        (normals [c,n,3], flags [c,n] i32: 1 = degenerate, normal (0,0,0))."""
        points = _chk(points, torch.float32, "points")
        if (neigh_multi is None) == (csr is None):
            raise EngineError("estimate_normals: exactly one of neigh_multi and csr expected")
        c, n, stride = points.shape
        normals = self._empty((c, n, 3))
        flags = self._empty((c, n), torch.int32)
        v = (C.c_float * 3)(*[float(x) for x in viewpoint])
        if csr is None:
            neigh_multi = _chk(neigh_multi, torch.int32, "neigh_idx")
            self._pre()
            self._call(self.lib.dsir_estimate_normals(self.h, _ptr(points), stride, _ptr(neigh_multi), neigh_multi.shape[1] * 16, c, n, v,
                                                      _ptr(normals), _ptr(flags)))
        else:
            off, cols = self._csr(csr, c * n, "estimate_normals")
            self._pre()
            self._call(self.lib.dsir_estimate_normals_csr(self.h, _ptr(points), stride, _ptr(off), _ptr(cols), c, n, v, _ptr(normals),
                                                          _ptr(flags)))
        self.sync()
        return normals, flags

    def _csr(self, csr, rows: int, who: str):
        """(offsets, cols) of a caller's CSR over ``rows`` rows, checked: the kernels trust the offsets, so a list that would leave cols
        is refused (two reductions and one read-back, no kernel work)."""
        off, cols = _chk(csr[0], torch.int32, "csr offsets"), _chk(csr[1], torch.int32, "csr cols")
        if off.numel() != rows + 1:
            raise EngineError(f"{who}: csr offsets must have clouds * n + 1 = {rows + 1} entries, got {off.numel()}")
        if int(off[0]) != 0 or int(off[-1]) != cols.numel() or bool((off[1:] < off[:-1]).any()):
            raise EngineError(f"{who}: csr offsets must start at 0, be non-decreasing and end at len(cols)")
        if cols.numel() == 0:                                       # every row empty: the kernels still want a pointer
            cols = torch.zeros((1,), dtype=torch.int32, device=self.device)
        return off, cols

    def fpfh(self, points, normals=None, neigh_multi=None, csr=None, pad_to: int = 64):
        """FPFH descriptors (include/dsir.h, dsir_fpfh; the rule: csrc/fpfh.hip, restated in deepsir_amd/fpfh.py): points [c,n,>=3],
        normals [c,n,3] (None: columns 3..5 of the rows) and exactly one of neigh_multi [c,S,16] (the pyramid's neigh_idx, its
        level-0 rows are read) and csr = (offsets [c n + 1] i32, cols i32 with cloud-local columns: what ``radius_matches(x, x,
        identity, r)`` returns) -> (desc [c,n,pad_to]: 33 values and zeros, pad_to = 64 feeds ``feature_correspondences``;
        flags [c,n] i32: 1 = no valid pair, the row is all zeros).  Needs no weights."""
        points = _chk(points, torch.float32, "points")
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[0] < 1 or points.shape[1] < 1:
            raise EngineError("fpfh: points [clouds >= 1, n >= 1, C >= 3] expected")
        c, n, stride = points.shape
        if normals is not None:
            normals = _chk(normals, torch.float32, "normals")
            if tuple(normals.shape) != (c, n, 3):
                raise EngineError(f"fpfh: normals must be [{c}, {n}, 3], got {tuple(normals.shape)}")
        if (neigh_multi is None) == (csr is None):
            raise EngineError("fpfh: exactly one of neigh_multi and csr expected")
        if pad_to < 33:
            raise EngineError("fpfh: pad_to >= 33 (the descriptor has 33 values)")
        neigh_cs, off, cols = 0, None, None
        if neigh_multi is not None:
            neigh_multi = _chk(neigh_multi, torch.int32, "neigh_idx")
            if neigh_multi.dim() != 3 or neigh_multi.shape[0] != c or neigh_multi.shape[1] < n or neigh_multi.shape[2] != 16:
                raise EngineError(f"fpfh: neigh_multi must be [{c}, >= {n}, 16], got {tuple(neigh_multi.shape)}")
            neigh_cs = neigh_multi.shape[1] * 16
        else:
            off, cols = self._csr(csr, c * n, "fpfh")
        desc = self._empty((c, n, int(pad_to)))
        flags = self._empty((c, n), torch.int32)
        self._pre()
        self._call(self.lib.dsir_fpfh(self.h, _ptr(points), stride, _ptr(normals), _ptr(neigh_multi), neigh_cs, _ptr(off), _ptr(cols),
                                      c, n, _ptr(desc), int(pad_to), _ptr(flags)))
        self.sync()
        return desc, flags

    def iss_keypoints(self, points, salient_radius=None, non_max_radius=None, gamma_21: float = 0.975, gamma_32: float = 0.975,
                      min_neighbors: int = 5, csr_salient=None, csr_nms=None):
        """ISS keypoints (include/dsir.h, dsir_iss_keypoints; the rule: csrc/iss.hip, restated in deepsir_amd/iss.py): points [c,n,>=3]
        and, for each of the two stages, exactly one of a radius (the CSR is then ``radius_neighbors(points, r, 0)``) and a CSR
        (offsets [c n + 1] i32, cols i32 with cloud-local columns, self included: what ``radius_neighbors`` returns) - the salient
        neighbourhoods whose covariance gives the saliency, and the non-max neighbourhoods a keypoint must dominate ->
        (index [c,n] i32: a cloud's keypoints in ascending point index, -1 beyond its count; counts [c] i32; saliency [c,n] f32;
        mask [c,n] i32).  Two radii build two cell indices (``NNIndex`` serves one radius).  Needs no weights.  Raises ValueError
        for arguments refused on the host (shapes, gammas, min_neighbors, the radius / CSR choice), EngineError where the library
        refuses."""
        points = _chk(points, torch.float32, "points")
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[0] < 1 or points.shape[1] < 1:
            raise ValueError("iss_keypoints: points [clouds >= 1, n >= 1, C >= 3] expected")
        for name, r, csr in (("salient", salient_radius, csr_salient), ("non_max", non_max_radius, csr_nms)):
            if (r is None) == (csr is None):
                raise ValueError(f"iss_keypoints: exactly one of {name}_radius and the {name} CSR expected")
        g21, g32 = float(gamma_21), float(gamma_32)
        if not (np.isfinite(g21) and g21 > 0.0 and np.isfinite(g32) and g32 > 0.0):
            raise ValueError(f"iss_keypoints: gamma_21 and gamma_32 must be finite and positive, got {gamma_21} and {gamma_32}")
        if int(min_neighbors) != min_neighbors or min_neighbors < 1 or min_neighbors > 0x7fffffff:
            raise ValueError(f"iss_keypoints: min_neighbors must be a positive int32, got {min_neighbors}")
        c, n, stride = points.shape
        if csr_salient is None:
            csr_salient = self.radius_neighbors(points, float(salient_radius), 0)
        if csr_nms is None:
            same = salient_radius is not None and float(non_max_radius) == float(salient_radius)
            csr_nms = csr_salient if same else self.radius_neighbors(points, float(non_max_radius), 0)
        so, sc = self._csr(csr_salient, c * n, "iss_keypoints")
        no, nc = (so, sc) if csr_nms is csr_salient else self._csr(csr_nms, c * n, "iss_keypoints")
        saliency = self._empty((c, n))
        mask, index = self._empty((c, n), torch.int32), self._empty((c, n), torch.int32)
        counts = self._empty((c,), torch.int32)
        self._pre()
        self._call(self.lib.dsir_iss_keypoints(self.h, _ptr(points), stride, _ptr(so), _ptr(sc), _ptr(no), _ptr(nc), c, n, g21, g32,
                                               int(min_neighbors), _ptr(saliency), _ptr(mask), _ptr(index), _ptr(counts)))
        self.sync()
        return index, counts, saliency, mask

    FPS_MAX_ROWS = 65536             # csrc/fps.h kFpsMaxRows: one workgroup per cloud

    def farthest_point_sample(self, points, k: int, counts=None, start: int = 0):
        """Farthest-point sampling (include/dsir.h, dsir_farthest_point_sample; the rule: csrc/fps.hip, restated in deepsir_amd/fps.py):
        points [c,cap,>=3], k rows per cloud, ``counts`` [c] (a device int32 tensor or a sequence; clouds of unequal sizes padded
        to one shape, harness.pad_clouds; None: every row), ``start`` the first row chosen where it exists and is finite ->
        (index [c,k] i32 in selection order, -1 beyond a cloud's count; counts_out [c] i32; min_d2 [c,k] f32: each chosen row's
        squared distance to the rows chosen before it, +inf for the first, 0 beyond the count).  Exactly k rows of a cloud with k
        finite rows and more, so what belongs to the rows (descriptors, normals, labels) rides along by a gather.  One workgroup
        per cloud, one launch; same bytes for a cloud alone or in a batch.  Needs no weights.  Raises ValueError for arguments
        refused on the host (shapes, k, start, counts, cap > 65536), EngineError where the library refuses."""
        points = _chk(points, torch.float32, "points")
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[0] < 1 or points.shape[1] < 1:
            raise ValueError("farthest_point_sample: points [clouds >= 1, cap >= 1, C >= 3] expected")
        c, cap, stride = points.shape
        if cap > self.FPS_MAX_ROWS:
            raise ValueError(f"farthest_point_sample: {cap} rows per cloud beyond the limit of {self.FPS_MAX_ROWS}")
        if int(k) != k or k < 1 or k > cap:
            raise ValueError(f"farthest_point_sample: k must be an integer in [1, {cap}] (the rows of the array), got {k}")
        if int(start) != start or start < 0 or start > 0x7fffffff:
            raise ValueError(f"farthest_point_sample: start must be a non-negative int32, got {start}")
        cn = self._counts(pair_counts(counts, c, cap, "counts"))
        index, min_d2 = self._empty((c, int(k)), torch.int32), self._empty((c, int(k)))
        counts_out = self._empty((c,), torch.int32)
        self._pre()
        self._call(self.lib.dsir_farthest_point_sample(self.h, _ptr(points), stride, _ptr(cn), c, cap, int(k), int(start), _ptr(index),
                                                       _ptr(counts_out), _ptr(min_d2)))
        self.sync()
        return index, counts_out, min_d2

    def segment_plane(self, points, distance_threshold: float, counts=None, hypotheses: int = 1024, max_planes: int = 1,
                      min_inliers: int = 3, axis=None, max_angle_deg=None, refine_iters: int = 1, seed: int = 0, cloud_ids=None):
        """RANSAC plane segmentation (include/dsir.h, dsir_segment_plane; the rule: csrc/plane.hip, restated in deepsir_amd/plane.py):
        points [c,cap,>=3], ``counts`` [c] as for ``farthest_point_sample``; per cloud up to ``max_planes`` planes are peeled, each
        the best of ``hypotheses`` three-row draws by its integer inlier count (|e| < distance_threshold), refitted ``refine_iters``
        times while the count does not drop; a cloud stops when no hypothesis is valid or the winner counts fewer than
        ``min_inliers``.  ``axis`` (3 numbers) orients the normals and, with ``max_angle_deg``, rejects planes whose normal is
        farther than that from it.  ``cloud_ids`` [c]: the id that enters each cloud's draws (None: its position), so that cloud c
        of a batch is cloud 0 of a call with seed ^ (c << 40).  -> (labels [c,cap] i32, -1 where no plane took the row; num_planes
        [c] i32; planes [c,max_planes,4] (n, d); anchors [c,max_planes,3]; plane_counts [c,max_planes] i32; stats
        [c,max_planes,4] i32 = winning hypothesis, valid hypotheses, count before the refits, refits kept), zeros at and behind
        num_planes.  Same bytes on every run and for a cloud alone or in a batch.  Needs no weights.  Raises ValueError for
        arguments refused on the host, EngineError where the library refuses."""
        from . import plane as _plane
        points = _chk(points, torch.float32, "points")
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[0] < 1 or points.shape[1] < 1:
            raise ValueError("segment_plane: points [clouds >= 1, cap >= 1, C >= 3] expected")
        c, cap, stride = points.shape
        if c > _plane.MAX_CLOUDS or c * cap >= 1 << 31:
            raise ValueError(f"segment_plane: clouds in [1, {_plane.MAX_CLOUDS}] with clouds x cap < 2^31 expected, got {c} x {cap}")
        thr = float(distance_threshold)
        if not (np.isfinite(np.float32(thr)) and np.float32(thr) > 0):
            raise ValueError(f"segment_plane: distance_threshold must be finite and positive in fp32, got {distance_threshold}")
        for name, v, lo, hi in (("hypotheses", hypotheses, 1, _plane.MAX_HYPOTHESES), ("max_planes", max_planes, 1, _plane.MAX_PLANES),
                                ("min_inliers", min_inliers, _plane.MIN_INLIERS, 0x7fffffff), ("refine_iters", refine_iters, 0, _plane.MAX_REFITS)):
            if int(v) != v or not lo <= v <= hi:
                raise ValueError(f"segment_plane: {name} must be an integer in [{lo}, {hi}], got {v}")
        if int(seed) != seed or not 0 <= seed < 1 << 64:
            raise ValueError(f"segment_plane: seed must be an unsigned 64-bit integer, got {seed}")
        try:
            ax, cos_min = _plane.axis_args(axis, max_angle_deg)
        except ValueError as e:
            raise ValueError(f"segment_plane: {e}") from None
        cn = self._counts(pair_counts(counts, c, cap, "counts"))
        ids = None
        if cloud_ids is not None:
            a = cloud_ids.detach().cpu().numpy() if isinstance(cloud_ids, torch.Tensor) else np.asarray(cloud_ids)
            if a.shape != (c,) or a.dtype.kind not in "iu" or (c and (int(a.min()) < 0 or int(a.max()) > 0x7fffffff)):
                raise ValueError(f"segment_plane: cloud_ids must hold {c} non-negative int32 values")
            ids = torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(self.device)
        m = int(max_planes)
        labels, num_planes = self._empty((c, cap), torch.int32), self._empty((c,), torch.int32)
        planes, anchors = self._empty((c, m, 4)), self._empty((c, m, 3))
        plane_counts, stats = self._empty((c, m), torch.int32), self._empty((c, m, 4), torch.int32)
        self._pre()
        self._call(self.lib.dsir_segment_plane(self.h, _ptr(points), stride, _ptr(cn), _ptr(ids), c, cap, thr, int(hypotheses), m,
                                               int(min_inliers), int(refine_iters), float(ax[0]), float(ax[1]), float(ax[2]), cos_min,
                                               int(seed), _ptr(labels), _ptr(num_planes), _ptr(planes), _ptr(anchors), _ptr(plane_counts),
                                               _ptr(stats)))
        self.sync()
        return labels, num_planes, planes, anchors, plane_counts, stats

    def score(self, feat, logits, xyz_multi, neigh_multi):
        """torch.max(logits) + score_fun counterpart -> (score [c,n], label [c,n] i32)."""
        feat, logits = _chk(feat, torch.float32, "feat"), _chk(logits, torch.float32, "logits")
        xyz_multi, neigh_multi = _chk(xyz_multi, torch.float32, "xyz"), _chk(neigh_multi, torch.int32, "neigh_idx")
        c, n, _ = feat.shape
        score = self._empty((c, n))
        label = self._empty((c, n), torch.int32)
        self._pre()
        self._call(self.lib.dsir_score(self.h, _ptr(feat), _ptr(logits), _ptr(xyz_multi), xyz_multi.shape[1] * 3,
                                       _ptr(neigh_multi), neigh_multi.shape[1] * 16, c, n, _ptr(score), _ptr(label)))
        self.sync()
        return score, label

    def aggregate(self, xyz, feat0, score):
        """One cloud-batch half of Network.aggregation -> desc [c,n,64]."""
        xyz, feat0, score = _chk(xyz, torch.float32, "xyz"), _chk(feat0, torch.float32, "feat0"), _chk(score, torch.float32, "score")
        c, n, _ = feat0.shape
        desc = self._empty((c, n, 64))
        self._pre()
        self._call(self.lib.dsir_aggregate(self.h, _ptr(xyz), xyz.shape[1] * 3, _ptr(feat0), _ptr(score), c, n, _ptr(desc)))
        self.sync()
        return desc

    def nn_match(self, desc_src, desc_ref, sync=True):
        """match_features_V2 + min(dim=2)[1] counterpart -> idx [p,J] i32."""
        desc_src, desc_ref = _chk(desc_src, torch.float32, "desc_src"), _chk(desc_ref, torch.float32, "desc_ref")
        p, J, _ = desc_src.shape
        K = desc_ref.shape[1]
        idx = self._empty((p, J), torch.int32)
        self._pre()
        self._call(self.lib.dsir_nn_match(self.h, _ptr(desc_src), _ptr(desc_ref), p, J, K, _ptr(idx)))
        if sync:
            self.sync()
        return idx

    def nn_match_screened(self, desc_src, desc_ref, want_stats=True):
        """Same arg-min as nn_match, computed the way dsir_register does (fp16-split screening + exact fp32 decision).
        Returns (idx [p,J] i32, (candidate entries emitted by the screening, rows left to the exhaustive kernel))."""
        desc_src, desc_ref = _chk(desc_src, torch.float32, "desc_src"), _chk(desc_ref, torch.float32, "desc_ref")
        p, J, _ = desc_src.shape
        K = desc_ref.shape[1]
        idx = self._empty((p, J), torch.int32)
        st = (C.c_int64 * 2)()
        self._pre()
        self._call(self.lib.dsir_nn_match_screened(self.h, _ptr(desc_src), _ptr(desc_ref), p, J, K, _ptr(idx),
                                                   st if want_stats else None))
        self.sync()
        return idx, (int(st[0]), int(st[1]))

    def screen_bounds(self, desc_src, desc_ref):
        """Diagnostics of the fp16 screening on one pair (include/dsir.h, dsir_screen_bounds): desc_src [J,64], desc_ref [K,64]
        -> dict(lower, upper, exact, zacc [J,K]; idx, thresh, cand_count [J]; cand_code, cand_lower [J,cap]; out_of_domain)."""
        a, b = _chk(desc_src, torch.float32, "desc_src"), _chk(desc_ref, torch.float32, "desc_ref")
        J, K = a.shape[0], b.shape[0]
        cap = int(self.lib.dsir_screen_cap())
        out = {"lower": self._empty((J, K)), "upper": self._empty((J, K)), "exact": self._empty((J, K)), "zacc": self._empty((J, K)),
               "idx": self._empty((J,), torch.int32), "thresh": self._empty((J,)), "cand_count": self._empty((J,), torch.int32),
               "cand_code": self._empty((J, cap), torch.int32), "cand_lower": self._empty((J, cap)),
               "out_of_domain": self._empty((1,), torch.int32)}
        self._pre()
        self._call(self.lib.dsir_screen_bounds(self.h, _ptr(a), _ptr(b), J, K, _ptr(out["lower"]), _ptr(out["upper"]),
                                               _ptr(out["exact"]), _ptr(out["zacc"]), _ptr(out["idx"]), _ptr(out["thresh"]), _ptr(out["cand_count"]),
                                               _ptr(out["cand_code"]), _ptr(out["cand_lower"]), _ptr(out["out_of_domain"])))
        self.sync()
        return out

    def kabsch(self, src, tgt, w):
        """compute_rigid_transform_2 counterpart -> (T [p,3,4], invalid [p] i32)."""
        src, tgt = _chk(src, torch.float32, "src"), _chk(tgt, torch.float32, "tgt")
        w = _chk(w.reshape(w.shape[0], -1), torch.float32, "weights")
        p, m, _ = src.shape
        T = self._empty((p, 3, 4))
        bad = self._empty((p,), torch.int32)
        self._pre()
        self._call(self.lib.dsir_kabsch(self.h, _ptr(src), _ptr(tgt), _ptr(w), p, m, _ptr(T), _ptr(bad)))
        self.sync()
        return T, bad

    # ------------------------------------------------------------------ the whole path
    def _pair_batch(self, points_src, points_ref, pyramids):
        """dsir_pair_batch of P pairs (+ the tensors that must stay alive while it is in use)."""
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        P, J, cin = points_src.shape
        K = points_ref.shape[1]
        if cin != self.cfg.feat_len or points_ref.shape[2] != cin:
            raise EngineError(f"points have {cin} channels, engine was built for feat_len={self.cfg.feat_len}")
        b = _lib.dsir_pair_batch()
        b.pairs, b.n_src, b.n_ref = P, J, K
        b.points_src, b.points_ref = _ptr(points_src), _ptr(points_ref)
        keep = [points_src, points_ref]
        if pyramids is not None:
            for side, fld in (("src", "src"), ("ref", "ref")):
                x = _chk(pyramids[f"points_{side}_xyz"], torch.float32, "xyz")
                nb = self.narrow(pyramids[f"points_{side}_neigh_idx"])
                sb = self.narrow(pyramids[f"points_{side}_sub_idx"])
                ip = self.narrow(pyramids[f"points_{side}_interp_idx"])
                keep += [x, nb, sb, ip]
                setattr(b, fld + "_xyz", _ptr(x)); setattr(b, fld + "_neigh", _ptr(nb))
                setattr(b, fld + "_sub", _ptr(sb)); setattr(b, fld + "_interp", _ptr(ip))
        return b, keep, (P, J, K)

    def register(self, points_src, points_ref, n_iter: int = 5, pyramids: Optional[dict] = None,
                 forced_idx: Optional[torch.Tensor] = None, want_aux: bool = True, sync: bool = True, out: Optional[dict] = None,
                 want_desc: bool = False):
        """forward_align_4 counterpart for P pairs.

        points_* [P, N, feat_len].  pyramids: optional dict with the reference's
        data-dict keys (points_{src,ref}_{xyz,neigh_idx,sub_idx,interp_idx}),
        int32 or int64.  Returns dict(transforms [P,n_iter,3,4], idx [n_iter,P,J],
        logits [n_iter,P,J], pt_ref_new [P,J,3], invalid [P])."""
        b, keep, (P, J, K) = self._pair_batch(points_src, points_ref, pyramids)
        if forced_idx is not None:
            forced_idx = _chk(forced_idx, torch.int32, "forced_idx")
            assert tuple(forced_idx.shape) == (n_iter, P, J)
            b.forced_idx = _ptr(forced_idx)
        if out is None:
            out = {"transforms": self._empty((P, n_iter, 3, 4))}
            if want_aux:
                out["idx"] = self._empty((n_iter, P, J), torch.int32)
                out["logits"] = self._empty((n_iter, P, J))
                out["pt_ref_new"] = self._empty((P, J, 3))
                out["invalid"] = self._empty((P,), torch.int32)
            if want_desc:     # test aid: the descriptors every iteration's search ran on
                out["desc_src"] = self._empty((n_iter, P, J, 64))
                out["desc_ref"] = self._empty((P, K, 64))
        r = _lib.dsir_pair_result()
        r.transforms = _ptr(out["transforms"])
        r.idx, r.logits = _ptr(out.get("idx")), _ptr(out.get("logits"))
        r.pt_ref_new, r.invalid = _ptr(out.get("pt_ref_new")), _ptr(out.get("invalid"))
        r.desc_src, r.desc_ref = _ptr(out.get("desc_src")), _ptr(out.get("desc_ref"))
        self._pre()
        self._call(self.lib.dsir_register(self.h, C.byref(b), n_iter, C.byref(r)))
        if sync:
            self.sync()
        out["_keep"] = keep
        return out

    def forward_pair(self, points_src, points_ref, num_sub: Optional[int] = None, pyramids: Optional[dict] = None,
                     sync: bool = True):
        """Network.forward_pair counterpart (reference model.py:609-666) for P pairs, point-major:
        returns {side: {xyz [P,M,3], feat [P,M,64], logits [P,N,ncls], score [P,M], label [P,M], index [P,M]}}
        with M = num_sub if num_sub > 0 else N; score/label/index only where the pipeline produces them."""
        num_sub = self.cfg.num_sub if num_sub is None else int(num_sub)
        b, keep, (P, J, K) = self._pair_batch(points_src, points_ref, pyramids)
        res, structs = {}, []
        for side, n in (("src", J), ("ref", K)):
            M = num_sub if num_sub > 0 else n
            o = {"xyz": self._empty((P, M, 3)), "feat": self._empty((P, M, 64)),
                 "logits": self._empty((P, n, self.cfg.num_classes))}
            if self.cfg.pipeline != "label":
                o["score"] = self._empty((P, M))
                o["label"] = self._empty((P, M), torch.int32)
                if num_sub > 0:
                    o["index"] = self._empty((P, M), torch.int32)
            c = _lib.dsir_cloud_out()
            for k in ("xyz", "feat", "logits", "score", "label", "index"):
                setattr(c, k, _ptr(o.get(k)))
            res[side] = o
            structs.append(c)
        self._pre()
        self._call(self.lib.dsir_forward_pair(self.h, C.byref(b), int(num_sub), C.byref(structs[0]), C.byref(structs[1])))
        if sync:
            self.sync()
        res["_keep"] = keep
        return res

    # ------------------------------------------------------------------ in front of the path: pre-processing
    def voxel_downsample(self, clouds: Sequence[torch.Tensor], voxel_size: float, crop: Optional[Sequence[float]] = None,
                         cap: Optional[int] = None):
        """open3d voxel_down_sample (+ process_point_cloud crop) counterpart for a ragged list of [n_i, C] CUDA
        clouds -> (voxels [clouds, cap, C], counts [clouds] i32).  See include/dsir.h for the ordering rule."""
        pts = torch.cat([_chk(c, torch.float32, "cloud") for c in clouds], 0)
        n = [int(c.shape[0]) for c in clouds]
        stride = pts.shape[1]
        offs = (C.c_int64 * (len(n) + 1))(*np.concatenate([[0], np.cumsum(n)]).tolist())
        cap = int(cap or max(n))
        out = self._empty((len(n), cap, stride))
        counts = self._empty((len(n),), torch.int32)
        crop_arr = None if crop is None else (C.c_float * 4)(*[float(x) for x in crop])
        self._pre()
        self._call(self.lib.dsir_voxel_downsample(self.h, _ptr(pts), offs, len(n), stride, float(voxel_size), crop_arr, cap,
                                                  _ptr(out), _ptr(counts)))
        return out, counts

    def resample(self, voxels: torch.Tensor, counts: torch.Tensor, k: int, seed: int = 0, mode: str = "random"):
        """Resampler / FixedResampler counterpart: [clouds, cap, C] + counts -> [clouds, k, C]."""
        voxels, counts = _chk(voxels, torch.float32, "voxels"), _chk(counts, torch.int32, "counts")
        c, cap, stride = voxels.shape
        out = self._empty((c, k, stride))
        self._pre()
        self._call(self.lib.dsir_resample(self.h, _ptr(voxels), _ptr(counts), c, cap, stride, int(k),
                                          {"random": 0, "fixed": 1}[mode], int(seed) & ((1 << 64) - 1), _ptr(out)))
        self.sync()
        return out

    def preprocess(self, clouds: Sequence[torch.Tensor], voxel_size: float, k: int, seed: int = 0,
                   crop: Optional[Sequence[float]] = None, mode: str = "random"):
        """Raw clouds -> [clouds, k, C] network input (crop, voxel average, resample in random order)."""
        vox, counts = self.voxel_downsample(clouds, voxel_size, crop)
        return self.resample(vox, counts, k, seed, mode), counts

    def augment(self, vox_src: torch.Tensor, counts_src: torch.Tensor, vox_ref: torch.Tensor, counts_ref: torch.Tensor, transform,
                cfg, seed: int, epoch: int, indices: Sequence[int], k: Optional[int] = None, return_rows: bool = False):
        """DataBase.apply_augment / apply_augment_V2 for P pairs on the device (csrc/augment.hip; the rule: deepsir_amd/augment.py).
        vox_* [P, cap, C] + counts_* [P] as ``voxel_downsample`` writes them, transform [P, 3|4, 4] (host, float64; None = identity),
        cfg an ``augment.AugmentConfig``, indices the samples' DATASET indices (the random keys come from (seed, epoch, index), never
        from the position in this call) -> (points_src [P,k,C], points_ref [P,k,C], transform_gt [P,3,4], invalid [2,P] i32: bit 0
        empty cloud, bit 1 non-finite centroid).  Host work: the per-cloud numbers, uploaded as ONE tensor; no synchronisation."""
        from . import augment as A
        ops = self._train_ops()
        P = len(indices)
        k = int(k or cfg.num_points)
        if k < 1:
            raise EngineError("augment: the number of output points (k or cfg.num_points) must be positive")
        M = np.tile(np.eye(4)[:3], (P, 1, 1)) if transform is None else np.asarray(transform, np.float64)[:, :3, :]
        pp = [A.pair_params(cfg, seed, epoch, int(i)) for i in indices]
        blocks = [A.pack_params([p[s] for p in pp]) for s in (0, 1)]
        host = np.concatenate([blocks[0].reshape(-1), blocks[1].reshape(-1), np.ascontiguousarray(M).reshape(-1)])
        dev = torch.from_numpy(host).to(self.device, non_blocking=True)
        n_prm = P * A.PARAM_SLOTS
        prm = (dev[:n_prm], dev[n_prm:2 * n_prm])
        cen = self._empty((2, P, 3), torch.float64)
        invalid = self._empty((2, P), torch.int32)
        out, rows = [], []
        for s, (vox, counts) in enumerate(((vox_src, counts_src), (vox_ref, counts_ref))):
            vox, counts = _chk(vox, torch.float32, "voxels"), _chk(counts, torch.int32, "counts")
            if vox.dim() != 3 or vox.shape[0] != P or counts.numel() != P or vox.shape[2] < 3:
                raise EngineError("augment: voxels [P, cap, C >= 3] and counts [P] expected for both sides")
            _, cap, stride = vox.shape
            sc = ops.scratch(max(int(self.lib.dsir_t_cloud_centroids_scratch(P)), int(self.lib.dsir_t_resample_keyed_scratch(P, cap))))
            ops._launch("dsir_t_cloud_centroids", _ptr(vox), _ptr(counts), P, cap, stride, _ptr(cen[s]), _ptr(invalid[s]), _ptr(sc))
            pts = self._empty((P, k, stride))
            r = self._empty((P, k), torch.int32) if return_rows else None
            need_perm = int(any(p[s].resample_mode != A.RESAMPLE_FIXED for p in pp))
            ops._launch("dsir_t_resample_keyed", _ptr(vox), _ptr(counts), P, cap, stride, k, _ptr(prm[s]), need_perm, _ptr(pts), _ptr(r),
                        _ptr(sc))
            ops._launch("dsir_t_augment", _ptr(pts), _ptr(counts), P, k, stride, _ptr(prm[s]), _ptr(cen[s]), _ptr(pts))
            out.append(pts)
            rows.append(r)
        gt = self._empty((P, 3, 4))
        ops._launch("dsir_t_augment_gt", _ptr(dev[2 * n_prm:]), _ptr(prm[0]), _ptr(prm[1]), _ptr(cen[0]), _ptr(cen[1]), P,
                    int(bool(cfg.reference_gt)), _ptr(gt))
        if return_rows:
            return out[0], out[1], gt, invalid, rows[0], rows[1]
        return out[0], out[1], gt, invalid

    def halfspace_crop(self, points: torch.Tensor, counts: torch.Tensor, p_keep, seed: int, epoch: int, indices: Sequence[int], sides,
                       out_cap: Optional[int] = None, directions=None):
        """Transforms.RandomCrop.crop for a ragged batch on the device (csrc/crop.hip; the rule: deepsir_amd/crop.py).  points
        [clouds, cap, C] + counts [clouds] i32, p_keep a float or one per cloud, indices the clouds' DATASET indices and sides their
        sides (an int or one per cloud): the direction of a cloud comes from (seed, epoch, index, side), never from its position in
        the call -> (out [clouds, out_cap, C]: the kept rows in input order, zeros behind them; out_counts [clouds] i32, which may
        exceed out_cap - then the first out_cap rows are written; invalid [clouds] i32: bit 0 nothing came in or is kept, bit 1
        non-finite centroid or threshold).  ``directions`` [clouds, 3] replaces the drawn ones.  Host work: the directions, uploaded
        as one tensor; no synchronisation."""
        from . import crop as K
        ops = self._train_ops()
        points, counts = _chk(points, torch.float32, "points"), _chk(counts, torch.int32, "counts")
        if points.dim() != 3 or points.shape[2] < 3 or counts.numel() != points.shape[0] or points.shape[0] < 1 or points.shape[1] < 1:
            raise EngineError("halfspace_crop: points [clouds >= 1, cap >= 1, C >= 3] and counts [clouds] expected")
        clouds, cap, stride = points.shape
        pk = np.ascontiguousarray(np.broadcast_to(np.asarray(p_keep, np.float64), (clouds,)))
        if not (np.isfinite(pk) & (pk > 0.0)).all():
            raise EngineError("halfspace_crop: every p_keep must be finite and > 0")
        sides = np.broadcast_to(np.asarray(sides, np.int64), (clouds,))
        if len(indices) != clouds:
            raise EngineError("halfspace_crop: one dataset index per cloud expected")
        dirs = K.crop_directions(seed, epoch, indices, sides) if directions is None else np.asarray(directions, np.float32)
        if dirs.shape != (clouds, 3):
            raise EngineError("halfspace_crop: directions [clouds, 3] expected")
        out_cap = int(out_cap or cap)
        dev = torch.from_numpy(np.ascontiguousarray(dirs)).to(self.device, non_blocking=True)
        cen = self._empty((clouds, 3), torch.float64)
        inv = self._empty((clouds,), torch.int32)
        out = torch.zeros((clouds, out_cap, stride), dtype=torch.float32, device=self.device)
        out_counts = self._empty((clouds,), torch.int32)
        nbytes = int(self.lib.dsir_t_halfspace_crop_scratch(clouds, cap))
        if nbytes == 0 or out_cap < 1:
            raise EngineError("halfspace_crop: shape refused (clouds * cap and clouds * out_cap must stay below 2^31, clouds <= 65535)")
        sc = ops.scratch(max(int(self.lib.dsir_t_cloud_centroids_scratch(clouds)), nbytes))
        ops._launch("dsir_t_cloud_centroids", _ptr(points), _ptr(counts), clouds, cap, stride, _ptr(cen), _ptr(inv), _ptr(sc))
        ops._launch("dsir_t_halfspace_crop", _ptr(points), _ptr(counts), clouds, cap, stride, _ptr(dev), pk.ctypes.data, _ptr(cen), out_cap,
                    _ptr(out), _ptr(out_counts), _ptr(inv), _ptr(sc))
        return out, out_counts, inv

    # ------------------------------------------------------------------ after the path: metrics
    METRIC_NAMES = ("r_mse", "r_mae", "t_mse", "t_mae", "err_r_deg", "err_t", "succ", "chamfer_dist")

    def eval_metrics(self, pred, gt, points_src, points_ref, rte_thresh: float, rre_thresh: float):
        """compute_metrics counterpart (reference common/metrics_util.py:27-85).
        pred [P,3,4] (may be a strided view such as transforms[:, i]), gt [P,3,4], points_* [P,N,>=3]
        -> dict of float64 tensors [P] keyed by METRIC_NAMES."""
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        gt = _chk(gt, torch.float32, "transform_gt")
        if not pred.is_cuda or pred.dtype != torch.float32 or pred.stride(-1) != 1 or pred.stride(-2) != 4:
            pred = pred.float().contiguous().to(self.device)
        P, n, stride = points_src.shape
        out = self._empty((P, 8), torch.float64)
        self._pre()
        self._call(self.lib.dsir_eval_metrics(self.h, _ptr(pred), pred.stride(0) if P > 1 else 12, _ptr(gt), _ptr(points_src),
                                              _ptr(points_ref), P, n, stride, float(rte_thresh), float(rre_thresh), _ptr(out)))
        self.sync()
        return {k: out[:, i] for i, k in enumerate(self.METRIC_NAMES)}

    # ------------------------------------------------------------------ measurement hooks
    ICP_ESTIMATORS = {"point": 0, "plane": 1}

    ICP_SEARCHES = ("brute", "grid", "auto")
    # search="auto" takes the cell index from this many reference points on: the measured crossover of tools/bench_icp.py's
    # single-pair sweep, rounded up to a power of two (profiles/README.md, "ICP: cell-indexed search")
    ICP_GRID_MIN_REF = 4096

    def _icp_search(self, search: str, K: int) -> int:
        """0 = brute force, 1 = cell index: a host-only decision on shapes, like the ones in csrc/search_plan.h"""
        if search not in self.ICP_SEARCHES:
            raise ValueError("search must be 'brute', 'grid' or 'auto'")
        return int(search == "grid" or (search == "auto" and K >= self.ICP_GRID_MIN_REF))

    def icp_refine(self, points_src, points_ref, T_init, max_corr_dist: float, max_iter: int = 30,
                   rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, estimator: str = "point", normals_ref=None,
                   viewpoint=(0.0, 0.0, 0.0), search: str = "brute", counts_src=None, counts_ref=None, kernel: str = "l2",
                   kernel_scale=None):
        """open3d registration_icp counterpart for P pairs (reference test.py:241-258, disabled there).
        points_* [P,N,>=3] CUDA fp32, T_init [P,3,4] -> (T [P,3,4], stats [P,4] f64: fitness, inlier_rmse, converged, iters).
        estimator="plane": the point-to-plane update (include/dsir.h, dsir_icp_refine_ex) and a fifth stats column, the identity
        updates taken for a singular system.  Its normals of points_ref: ``normals_ref`` [P,K,3] if given, else columns 3..5 of
        rows of 6 columns and more (the use_ppf layout), else estimated here - knn_pyramid on points_ref, estimate_normals on its
        level-0 lists towards ``viewpoint`` - which needs a cloud the pyramid accepts (ValueError otherwise).
        search: "brute" (J x K distance tests per iteration), "grid" (a cell index of points_ref built once per call,
        csrc/icp_grid.hip) or "auto" (the grid from ICP_GRID_MIN_REF reference points on).  Same bytes out, whichever is taken.
        counts_src / counts_ref: [P] int32 device tensors or sequences, the rows of each pair that hold points (clouds of unequal
        sizes padded to one shape, harness.pad_clouds); None: all of them.  Rows beyond a count are never read, and pair p gets,
        byte for byte, what the call on points_src[p:p+1, :counts_src[p]], points_ref[p:p+1, :counts_ref[p]] alone returns.  A
        count outside [0, rows] is a ValueError.  With counts_ref the plane estimator's normals are not estimated here (the
        pyramid takes dense clouds): pass normals_ref, or rows that carry them.
        kernel / kernel_scale: open3d's ``robust_kernel`` of the estimator (include/dsir.h, dsir_icp_refine_ex4): "l2" (every
        correspondence weighs 1; the scale is ignored), "huber", "cauchy", "gm" or "tukey" with a finite scale k > 0 in the cloud's
        length unit (ValueError otherwise).  It weighs the update alone; search, stats and the convergence test do not see it."""
        if estimator not in self.ICP_ESTIMATORS:
            raise ValueError("estimator must be 'point' or 'plane'")
        kern, scale = icp_kernel_args(kernel, kernel_scale)
        grid = self._icp_search(search, points_ref.shape[1])
        P, J, stride = points_src.shape
        K = points_ref.shape[1]
        counts_src, counts_ref = pair_counts(counts_src, P, J, "counts_src"), pair_counts(counts_ref, P, K, "counts_ref")
        if estimator == "plane" and counts_ref is not None and normals_ref is None and stride < 6:
            raise ValueError("estimator='plane' with counts_ref does not estimate the normals (the KNN pyramid takes dense clouds): "
                             "pass normals_ref [P,K,3], or rows that carry the normals in columns 3..5")
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        T_init = _chk(T_init, torch.float32, "T_init")
        assert points_ref.shape[0] == P and points_ref.shape[2] == stride and tuple(T_init.shape) == (P, 3, 4)
        plane = self.ICP_ESTIMATORS[estimator]
        if not plane:
            normals_ref = None
        elif normals_ref is not None:
            normals_ref = _chk(normals_ref, torch.float32, "normals_ref")
            if tuple(normals_ref.shape) != (P, K, 3):
                raise ValueError(f"normals_ref must be [{P}, {K}, 3], got {tuple(normals_ref.shape)}")
        elif stride < 6:
            normals_ref = self.icp_normals(points_ref, viewpoint)
        T = self._empty((P, 3, 4))
        stats = self._empty((P, 5), torch.float64)
        args = (self.h, _ptr(points_src), _ptr(points_ref), P, J, K, stride, float(max_corr_dist), int(max_iter), float(rel_fitness),
                float(rel_rmse), _ptr(T_init), _ptr(T), plane, _ptr(normals_ref), grid, _ptr(stats))
        cs, cr = self._counts(counts_src), self._counts(counts_ref)
        self._pre()
        if kern:
            self._call(self.lib.dsir_icp_refine_ex4(*args, _ptr(cs), _ptr(cr), kern, scale))
        elif cs is None and cr is None:
            self._call(self.lib.dsir_icp_refine_ex2(*args))
        else:
            self._call(self.lib.dsir_icp_refine_ex3(*args, _ptr(cs), _ptr(cr)))
        self.sync()
        return T, (stats if plane else stats[:, :4].contiguous())

    def _counts(self, host):
        """pair_counts' array on the device (None stays None)"""
        return None if host is None else torch.from_numpy(host).to(self.device)

    def ndt_refine(self, points_src, points_ref, T_init, resolution: float, neighbors: int = 7, max_iter: int = 30,
                   step_tol: float = 1e-4, outlier_ratio: float = 0.55, counts_src=None, counts_ref=None):
        """NDT registration for P pairs (include/dsir.h, dsir_ndt_refine; the rule: csrc/ndt.hip, restated in deepsir_amd/ndt.py):
        the reference cloud as one Gaussian per occupied cell of edge ``resolution``, the source points pulled towards the Gaussians
        of their own and (``neighbors=7``) face-adjacent cells - no nearest-neighbour search, no normals, a wider basin than ICP on
        sparse scans.  points_* [P,N,>=3] CUDA fp32, T_init [P,3,4] -> (T [P,3,4], stats [P,5] fp32: mean likelihood, matched
        fraction, converged, iterations, identity updates).  ``step_tol``: a pair stops when its update turns by less than that
        (radians) and shifts by less than step_tol x resolution.  counts_src / counts_ref as for ``icp_refine``: pair p gets, byte
        for byte, what the call on its own rows alone returns.  A bad argument is an EngineError and leaves the engine usable."""
        P, J, stride = points_src.shape
        K = points_ref.shape[1]
        counts_src, counts_ref = pair_counts(counts_src, P, J, "counts_src"), pair_counts(counts_ref, P, K, "counts_ref")
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        T_init = _chk(T_init, torch.float32, "T_init")
        assert points_ref.shape[0] == P and points_ref.shape[2] == stride and tuple(T_init.shape) == (P, 3, 4)
        T = self._empty((P, 3, 4))
        stats = self._empty((P, 5))
        cs, cr = self._counts(counts_src), self._counts(counts_ref)
        self._pre()
        self._call(self.lib.dsir_ndt_refine(self.h, _ptr(points_src), _ptr(points_ref), P, J, K, stride, _ptr(cs), _ptr(cr), _ptr(T_init),
                                            float(resolution), int(neighbors), int(max_iter), float(step_tol), float(outlier_ratio),
                                            _ptr(T), _ptr(stats)))
        self.sync()
        return T, stats

    def ndt_map(self, points_ref, resolution: float, counts_ref=None):
        """The map ``ndt_refine`` builds of points_ref [P,K,>=3] (include/dsir.h, dsir_ndt_map) -> (lattice [P,4] f64: origin and
        cell edge; keys [P,K] int64: the sorted cell keys, -1 (all ones) for non-finite and padding rows; index [P,K] i32: the
        original row of every sorted position; records [P,K,10] f64: mean, inverse covariance (00 01 02 11 12 22) and point count
        at the first sorted position of every valid cell, zero elsewhere)."""
        P, K, stride = points_ref.shape
        counts_ref = pair_counts(counts_ref, P, K, "counts_ref")
        points_ref = _chk(points_ref, torch.float32, "points_ref")
        lattice = self._empty((P, 4), torch.float64)
        keys = self._empty((P, K), torch.int64)
        index = self._empty((P, K), torch.int32)
        records = self._empty((P, K, 10), torch.float64)
        cr = self._counts(counts_ref)
        self._pre()
        self._call(self.lib.dsir_ndt_map(self.h, _ptr(points_ref), P, K, stride, _ptr(cr), float(resolution), _ptr(lattice), _ptr(keys),
                                         _ptr(index), _ptr(records)))
        self.sync()
        return lattice, keys, index, records

    def icp_correspondences(self, points_src, points_ref, T, max_corr_dist: float, search: str = "brute", counts_src=None, counts_ref=None):
        """open3d evaluate_registration counterpart for P pairs: one search step of icp_refine under the pose T.
        points_* [P,N,>=3] CUDA fp32, T [P,3,4] -> (idx [P,J] i32: the reference point of each source point moved by T, or -1;
        d2 [P,J] fp32: its squared distance, 0 where idx is -1; stats [P,2] f64: fitness, inlier_rmse).  search and counts_* as for
        icp_refine; entries of idx and d2 at and beyond a pair's counts_src are -1 and 0, its fitness is matched / counts_src."""
        grid = self._icp_search(search, points_ref.shape[1])
        P, J, stride = points_src.shape
        K = points_ref.shape[1]
        counts_src, counts_ref = pair_counts(counts_src, P, J, "counts_src"), pair_counts(counts_ref, P, K, "counts_ref")
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        T = _chk(T, torch.float32, "T")
        assert points_ref.shape[0] == P and points_ref.shape[2] == stride and tuple(T.shape) == (P, 3, 4)
        idx, d2 = self._empty((P, J), torch.int32), self._empty((P, J))
        stats = self._empty((P, 2), torch.float64)
        args = (self.h, _ptr(points_src), _ptr(points_ref), P, J, K, stride, float(max_corr_dist), _ptr(T), grid, _ptr(idx), _ptr(d2), _ptr(stats))
        cs, cr = self._counts(counts_src), self._counts(counts_ref)
        self._pre()
        if cs is None and cr is None:
            self._call(self.lib.dsir_icp_correspondences(*args))
        else:
            self._call(self.lib.dsir_icp_correspondences_ex(*args, _ptr(cs), _ptr(cr)))
        self.sync()
        return idx, d2, stats

    def information_matrix(self, points_src, points_ref, T, max_corr_dist: float, search: str = "brute", counts_src=None, counts_ref=None):
        """open3d get_information_matrix_from_point_clouds counterpart for P pairs (include/dsir.h, dsir_information_matrix).
        Arguments as for icp_correspondences, whose correspondence set this sums over -> (info [P,6,6] f64 in the order
        [rotation; translation], symmetric; count [P] i32: the correspondences).  Same bytes for every ``search``; counts_* as for
        icp_refine (include/dsir.h, dsir_information_matrix_ex)."""
        grid = self._icp_search(search, points_ref.shape[1])
        P, J, stride = points_src.shape
        K = points_ref.shape[1]
        counts_src, counts_ref = pair_counts(counts_src, P, J, "counts_src"), pair_counts(counts_ref, P, K, "counts_ref")
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        T = _chk(T, torch.float32, "T")
        assert points_ref.shape[0] == P and points_ref.shape[2] == stride and tuple(T.shape) == (P, 3, 4)
        info, count = self._empty((P, 6, 6), torch.float64), self._empty((P,), torch.int32)
        args = (self.h, _ptr(points_src), _ptr(points_ref), P, J, K, stride, float(max_corr_dist), _ptr(T), grid, _ptr(info), _ptr(count))
        cs, cr = self._counts(counts_src), self._counts(counts_ref)
        self._pre()
        if cs is None and cr is None:
            self._call(self.lib.dsir_information_matrix(*args))
        else:
            self._call(self.lib.dsir_information_matrix_ex(*args, _ptr(cs), _ptr(cr)))
        self.sync()
        return info, count

    def pose_graph_optimize(self, graphs, max_iter: int = 100):
        """open3d global_optimization counterpart for a list of graphs, one workgroup each (include/dsir.h,
        dsir_pose_graph_optimize).  graphs: ``pose_graph.PoseGraph`` objects or dicts with their fields (X0 [N,3,4], st [E,2],
        T [E,3,4], info [E,6,6], uncertain [E], mu, reference_node), numpy on the host; they are checked (ValueError: more than
        128 nodes, disconnected, no edge, bad reference node - before any launch) and packed CSR-style here.
        -> list of (X [N,3,4] f64, line [E] f64, stats [4] f64: F at X0, F at X, solves, status) as numpy, one per graph."""
        from . import pose_graph as PG
        p = PG.pack_graphs(graphs)
        G = len(p["mu"])
        i32p = lambda a: a.ctypes.data_as(_lib.c_i32_p)
        nbytes = self.lib.dsir_pose_graph_scratch_bytes(G, i32p(p["node_off"]), i32p(p["edge_off"]), i32p(p["reference_node"]))
        if nbytes == 0:
            raise EngineError("dsir_pose_graph_scratch_bytes: the batch is refused")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        X0, st, T, info, unc, mu = (dev(p[k]) for k in ("X0", "st", "T", "info", "uncertain", "mu"))
        scratch = self._empty(((nbytes + 7) // 8,), torch.float64)
        X, line = torch.empty_like(X0), self._empty((max(int(p["edge_off"][-1]), 1),), torch.float64)
        stats = self._empty((G, 4), torch.float64)
        self._pre()
        self._call(self.lib.dsir_pose_graph_optimize(self.h, G, i32p(p["node_off"]), i32p(p["edge_off"]), _ptr(X0), _ptr(st), _ptr(T),
                                                     _ptr(info), _ptr(unc), _ptr(mu), i32p(p["reference_node"]), int(max_iter),
                                                     _ptr(scratch), _ptr(X), _ptr(line), _ptr(stats)))
        self.sync()
        X, line, stats = X.cpu().numpy(), line.cpu().numpy(), stats.cpu().numpy()
        no, eo = p["node_off"], p["edge_off"]
        return [(X[no[g]:no[g + 1]], line[eo[g]:eo[g + 1]], stats[g]) for g in range(G)]

    def icp_normals(self, points_ref, viewpoint=(0.0, 0.0, 0.0)):
        """The normals icp_refine(estimator="plane") estimates when it is given none: knn_pyramid on points_ref [P,K,>=3], then
        estimate_normals on the level-0 lists -> [P,K,3].  ValueError for a cloud the pyramid does not accept."""
        K = points_ref.shape[1]
        if K > self.max_points or level_sizes(K, self.cfg.sub_sampling_ratio)[len(self.cfg.d_out) - 1] < self.cfg.num_knn:
            raise ValueError(f"estimator='plane' cannot estimate normals for a reference cloud of {K} points (the KNN pyramid takes "
                             f"{64 * self.cfg.num_knn} .. max_points={self.max_points}): pass normals_ref, or rows that carry the "
                             "normals in columns 3..5")
        _, neigh, _, _ = self.knn_pyramid(points_ref)
        return self.estimate_normals(points_ref, neigh, viewpoint)[0]

    def _correspondence_pose(self, name, points_src, points_ref, corr, counts, T_init, scalars, diag_type, diag_table, diag):
        """What ransac_ / consensus_ / fgr_correspondence share: the tensor checks under the method's ``name``, the outputs, with ``diag``
        the diagnostics of ``diag_table`` (key, shape after P, dtype; the fields of ``diag_type`` in order), the call (``scalars``: M .. T_init)."""
        points_src, points_ref = _chk(points_src, torch.float32, "points_src"), _chk(points_ref, torch.float32, "points_ref")
        corr = _chk(corr, torch.int32, "corr")
        P, J, stride = points_src.shape
        K, M = points_ref.shape[1], corr.shape[1]
        if points_ref.shape[0] != P or points_ref.shape[2] != stride or tuple(corr.shape) != (P, M, 2):
            raise EngineError(f"{name}: points_* must be [P,N,stride] and corr [P,M,2]")
        if counts is not None:
            counts = _chk(counts, torch.int32, "counts")
            if tuple(counts.shape) != (P,):
                raise EngineError(f"{name}: counts must be [P]")
        if T_init is not None:
            T_init = _chk(T_init, torch.float32, "T_init")
            if tuple(T_init.shape) != (P, 3, 4):
                raise EngineError(f"{name}: T_init must be [P,3,4]")
        T = self._empty((P, 3, 4))
        stats = self._empty((P, 5), torch.float64)
        invalid = self._empty((P,), torch.int32)
        d, dref = None, None
        if diag:
            d = {k: self._empty((P,) + shape, dtype) for k, shape, dtype in diag_table}
            dref = C.byref(diag_type(*[_ptr(v) for v in d.values()]))
        self._pre()
        self._call(getattr(self.lib, "dsir_" + name)(self.h, _ptr(points_src), _ptr(points_ref), P, J, K, stride, _ptr(corr), _ptr(counts),
                                                     M, *scalars, _ptr(T_init), _ptr(T), _ptr(stats), _ptr(invalid), dref))
        self.sync()
        return (T, stats, invalid, d) if diag else (T, stats, invalid)

    RANSAC_CHUNK = 256                 # DSIR_RANSAC_CHUNK: correspondences a scoring workgroup stages per step
    RANSAC_MAX_HYPOTHESES = 1 << 20    # DSIR_RANSAC_MAX_HYPOTHESES

    def ransac_correspondence(self, points_src, points_ref, corr, max_dist: float, counts=None, ransac_n: int = 3,
                              edge_sim: float = 0.9, hypotheses: int = 8192, refine_iters: int = 2, seed: int = 0, T_init=None,
                              diag: bool = False):
        """open3d registration_ransac_based_on_correspondence counterpart for P pairs (reference network/DGR.py:26-36, :249-306;
        parity unpinned, the rule is stated in csrc/ransac.hip and restated in deepsir_amd/ransac.py).
        points_* [P,N,>=3] CUDA fp32, corr [P,M,2] i32 (src index, ref index), counts [P] i32 or None, T_init [P,3,4] or None
        -> (T [P,3,4], stats [P,5] f64: fitness, inlier_rmse, winning hypothesis or -1, valid hypotheses, inliers; invalid [P] i32)
        and, with diag=True, a dict of hyp_sample [P,H,4], hyp_T [P,H,3,4], hyp_valid [P,H], hyp_count [P,H]."""
        Hn, i32 = max(int(hypotheses), 1), torch.int32
        table = [("hyp_sample", (Hn, 4), i32), ("hyp_T", (Hn, 3, 4), torch.float32), ("hyp_valid", (Hn,), i32), ("hyp_count", (Hn,), i32)]
        scalars = (float(max_dist), int(ransac_n), float(edge_sim), int(hypotheses), int(refine_iters), int(seed) & ((1 << 64) - 1))
        return self._correspondence_pose("ransac_correspondence", points_src, points_ref, corr, counts, T_init, scalars,
                                    _lib.dsir_ransac_diag, table, diag)

    CONSENSUS_MAX_SEEDS = 256          # DSIR_CONSENSUS_MAX_SEEDS
    CONSENSUS_MAX_MEMBERS = 128        # DSIR_CONSENSUS_MAX_MEMBERS
    CONSENSUS_MAX_M = 24576            # DSIR_CONSENSUS_MAX_M

    def consensus_correspondence(self, points_src, points_ref, corr, max_dist: float, counts=None, compat_dist=None, seeds: int = 64,
                                 members: int = 32, refine_iters: int = 2, T_init=None, diag: bool = False):
        """Spatial-consensus pose for P pairs: the deterministic alternative to ransac_correspondence for correspondence sets that are
        mostly wrong (parity unpinned, the rule is stated in csrc/consensus.hip and restated in deepsir_amd/consensus.py).
        Arguments and results as ransac_correspondence; compat_dist None / <= 0: max_dist.
        -> (T [P,3,4], stats [P,5] f64: fitness, inlier_rmse, winning seed rank or -1, valid seeds, inliers; invalid [P] i32) and, with
        diag=True, a dict of bits [P,M,W] i64 (the words of the compatibility matrix), score [P,M] i32, seed [P,seeds],
        seed_members [P,seeds,members], seed_T [P,seeds,3,4], seed_valid [P,seeds], seed_count [P,seeds]."""
        Hn, Mn = min(max(int(seeds), 1), self.CONSENSUS_MAX_SEEDS), min(max(int(members), 1), self.CONSENSUS_MAX_MEMBERS)
        M, i32 = corr.shape[1], torch.int32
        table = [("bits", (M, (M + 63) // 64), torch.int64), ("score", (M,), i32), ("seed", (Hn,), i32), ("seed_members", (Hn, Mn), i32),
                 ("seed_T", (Hn, 3, 4), torch.float32), ("seed_valid", (Hn,), i32), ("seed_count", (Hn,), i32)]
        scalars = (float(max_dist), float(compat_dist or 0.0), int(seeds), int(members), int(refine_iters))
        return self._correspondence_pose("consensus_correspondence", points_src, points_ref, corr, counts, T_init, scalars,
                                    _lib.dsir_consensus_diag, table, diag)

    FGR_MAX_TUPLES = 65536             # DSIR_FGR_MAX_TUPLES
    FGR_MAX_TRIALS = 1 << 22           # DSIR_FGR_MAX_TRIALS
    FGR_MAX_ITERS = 1024               # DSIR_FGR_MAX_ITERS

    def fgr_correspondence(self, points_src, points_ref, corr, max_dist: float, counts=None, tuple_test: bool = True,
                           tuple_scale: float = 0.95, max_tuples: int = 1000, max_trials: int = 1 << 20, iterations: int = 64,
                           division_factor: float = 1.4, refine_iters: int = 2, seed: int = 0, T_init=None, diag: bool = False):
        """Fast global registration pose for P pairs (open3d registration_fgr_based_on_feature_matching's estimator on an explicit
        correspondence list; parity unpinned, the rule is stated in csrc/fgr.hip and restated in deepsir_amd/fgr.py): a tuple
        pre-filter, then ``iterations`` Gauss-Newton steps under a graduated robust weight - no hypotheses, no quadratic memory.
        Arguments and results as ransac_correspondence.
        -> (T [P,3,4], stats [P,5] f64: fitness, inlier_rmse, 0 or -1 (no pose), 1 or 0, inliers; invalid [P] i32) and, with
        diag=True, a dict of rows [P,L] i32 (L = 3 max_tuples, or M without the tuple test; -1 padded), n_rows [P], trials [P],
        norm [P,8] f64 (ms, mq, scale), iter_T [P,iterations,3,4] f64, iter_mu / iter_energy [P,iterations] f64, iters_run [P]."""
        L = 3 * min(max(int(max_tuples), 1), self.FGR_MAX_TUPLES) if tuple_test else corr.shape[1]
        It, i32, f64 = min(max(int(iterations), 1), self.FGR_MAX_ITERS), torch.int32, torch.float64
        table = [("rows", (L,), i32), ("n_rows", (), i32), ("trials", (), i32), ("norm", (8,), f64), ("iter_T", (It, 3, 4), f64),
                 ("iter_mu", (It,), f64), ("iter_energy", (It,), f64), ("iters_run", (), i32)]
        scalars = (float(max_dist), 1 if tuple_test else 0, float(tuple_scale), int(max_tuples), int(max_trials), int(iterations),
                   float(division_factor), int(refine_iters), int(seed) & ((1 << 64) - 1))
        return self._correspondence_pose("fgr_correspondence", points_src, points_ref, corr, counts, T_init, scalars, _lib.dsir_fgr_diag,
                                    table, diag)

    def feature_correspondences(self, desc_src, desc_ref, mutual: bool = True, k: int = 1, ratio: float = 0.0, with_dist: bool = False):
        """The correspondence set of open3d's registration_ransac_based_on_feature_matching (reference network/DGR.py:7-24),
        made explicit: exact descriptor arg-min src -> ref (nn_match), kept where the ref -> src arg-min points back (mutual),
        in ascending src index.  desc_* [P,N,64] -> (corr [P,J,2] i32 with -1 beyond counts[p], counts [P] i32).
        k > 1: the k nearest ref descriptors of every src row as candidates (corr [P,J*k,2], ascending j then rank; mutual: j
        among the k nearest of the candidate's column).  ratio in (0, 1): Lowe's ratio test on the 1-NN set (k must be 1).  with_dist:
        also the kept distances [P,J*k] f32 (+inf beyond counts[p]).  The rule: include/dsir.h, dsir_feature_correspondences_ex."""
        desc_src, desc_ref = _chk(desc_src, torch.float32, "desc_src"), _chk(desc_ref, torch.float32, "desc_ref")
        P, J, c = desc_src.shape
        K = desc_ref.shape[1]
        if c != 64 or desc_ref.shape[0] != P or desc_ref.shape[2] != 64:
            raise EngineError("feature_correspondences: descriptors must be [P,N,64]")
        k, ratio = int(k), float(ratio)
        if k == 1 and ratio == 0.0 and not with_dist:
            corr = self._empty((P, J, 2), torch.int32)
            counts = self._empty((P,), torch.int32)
            self._pre()
            self._call(self.lib.dsir_feature_correspondences(self.h, _ptr(desc_src), _ptr(desc_ref), P, J, K, 1 if mutual else 0,
                                                             _ptr(corr), _ptr(counts)))
            self.sync()
            return corr, counts
        M = J * max(k, 1)
        corr = self._empty((P, M, 2), torch.int32)
        counts = self._empty((P,), torch.int32)
        dist = self._empty((P, M)) if with_dist else None
        self._pre()
        self._call(self.lib.dsir_feature_correspondences_ex(self.h, _ptr(desc_src), _ptr(desc_ref), P, J, K, 1 if mutual else 0, k, ratio,
                                                            _ptr(corr), _ptr(counts), _ptr(dist)))
        self.sync()
        return (corr, counts, dist) if with_dist else (corr, counts)

    def nn_match_topk(self, desc_src, desc_ref, k: int, with_dist: bool = True):
        """The k nearest ref descriptors of every src descriptor, ascending by (fp32 distance, column); rank 0 is nn_match's result.
        desc_* [P,N,64] -> (idx [P,J,k] i32, dist [P,J,k] f32 or None); ranks beyond K are -1 / +inf (include/dsir.h)."""
        desc_src, desc_ref = _chk(desc_src, torch.float32, "desc_src"), _chk(desc_ref, torch.float32, "desc_ref")
        P, J, c = desc_src.shape
        K = desc_ref.shape[1]
        if c != 64 or desc_ref.shape[0] != P or desc_ref.shape[2] != 64:
            raise EngineError("nn_match_topk: descriptors must be [P,N,64]")
        k = int(k)
        idx = self._empty((P, J, max(k, 1)), torch.int32)
        dist = self._empty((P, J, max(k, 1))) if with_dist else None
        self._pre()
        self._call(self.lib.dsir_nn_match_topk(self.h, _ptr(desc_src), _ptr(desc_ref), P, J, K, k, _ptr(idx), _ptr(dist)))
        self.sync()
        return idx, dist

    def nn_match_topk_splits(self, pairs: int, J: int, K: int, k: int) -> int:
        """Column splits the top-k launcher takes for this shape (host arithmetic)."""
        return int(self.lib.dsir_nn_match_topk_splits(self.h, int(pairs), int(J), int(K), int(k)))

    def pose_finetune(self, xyz_src, xyz_ref, T_init, weights=None, weights_are_logits: bool = False,
                      quantization_size: float = 1.0, max_iter: int = 1000, break_threshold_ratio: float = 1e-4,
                      max_break_count: int = 20):
        """transformation_finetune counterpart for P pairs (reference test.py:159-207, disabled there).
        xyz_src / xyz_ref [P,m,3] matched points, T_init [P,3,4], weights [P,m] or None
        -> (T [P,3,4], stats [P,3] f64: iterations, loss, break_count)."""
        xyz_src, xyz_ref = _chk(xyz_src, torch.float32, "xyz_src"), _chk(xyz_ref, torch.float32, "xyz_ref")
        T_init = _chk(T_init, torch.float32, "T_init")
        P, m, three = xyz_src.shape
        if three != 3 or tuple(xyz_ref.shape) != (P, m, 3) or tuple(T_init.shape) != (P, 3, 4):
            raise EngineError("pose_finetune: xyz_src / xyz_ref must be [P,m,3] and T_init [P,3,4]")
        if weights is not None:
            weights = _chk(weights.reshape(P, -1), torch.float32, "weights")
            if weights.shape[1] != m:
                raise EngineError("pose_finetune: weights must be [P,m]")
        T = self._empty((P, 3, 4))
        stats = self._empty((P, 3), torch.float64)
        self._pre()
        self._call(self.lib.dsir_pose_finetune(self.h, _ptr(xyz_src), _ptr(xyz_ref), _ptr(weights), 1 if weights_are_logits else 0,
                                               P, m, _ptr(T_init), float(quantization_size), int(max_iter),
                                               float(break_threshold_ratio), int(max_break_count), _ptr(T), _ptr(stats)))
        self.sync()
        return T, stats

    def align_loss_backward(self, pt_src, pt_ref, idx, logits, labels, transform_gt, loss_type: str = "mae",
                            wt_ptDist_loss: float = 1.0, wt_inlier_loss: float = 1.0, loss_discount_factor: float = 0.5,
                            per_pair: bool = False, wt_pose_loss: float = 0.0):
        """ScanAlignmentLoss (reduction='mean') + its gradient down to the inlier logits (include/dsir.h).
        pt_src [P,J,3], pt_ref [P,K,3], idx [n,P,J] i32, logits [n,P,J], labels [n,P,J] or None, transform_gt [P,3,4]
        -> dict(losses {mae_i|mse_i, outlier_i, total}, grad_logits [n,P,J], transforms [P,n,3,4]).
        wt_pose_loss > 0 adds the rotation + translation error term (loss.py:830-842): keys poseError_i, as the reference's dict has
        them only then (dsir_align_loss_backward3; 0 runs dsir_align_loss_backward2 as before).  With wt_ptDist_loss == 0 the
        keys mae_i | mse_i stay, at 0, as in the reference (loss.py:793-798)."""
        pt_src, pt_ref = _chk(pt_src, torch.float32, "pt_src"), _chk(pt_ref, torch.float32, "pt_ref")
        idx, logits = _chk(idx, torch.int32, "idx"), _chk(logits, torch.float32, "logits")
        transform_gt = _chk(transform_gt, torch.float32, "transform_gt")
        if labels is not None:
            labels = _chk(labels, torch.float32, "labels")
        n, P, J = logits.shape
        K = pt_ref.shape[1]
        if tuple(pt_src.shape) != (P, J, 3) or tuple(idx.shape) != (n, P, J) or tuple(transform_gt.shape) != (P, 3, 4) or \
                (labels is not None and tuple(labels.shape) != (n, P, J)):
            raise EngineError("align_loss_backward: inconsistent shapes")
        lt = {"mae": 0, "mse": 1}[loss_type]
        wt_pose_loss = check_pose_weight(wt_pose_loss)
        pose = wt_pose_loss > 0.0
        nc = 3 if pose else 2
        T = self._empty((P, n, 3, 4))
        grad = self._empty((n, P, J))
        losses = (C.c_double * (nc * n))()
        pp = (C.c_double * (nc * n * P))() if per_pair else None
        self._pre()
        if pose:
            self._call(self.lib.dsir_align_loss_backward3(self.h, _ptr(pt_src), _ptr(pt_ref), _ptr(idx), _ptr(logits), _ptr(labels),
                                                          _ptr(transform_gt), P, J, K, n, lt, float(wt_ptDist_loss), float(wt_inlier_loss),
                                                          float(loss_discount_factor), wt_pose_loss, _ptr(T), losses, _ptr(grad), pp))
        else:
            self._call(self.lib.dsir_align_loss_backward2(self.h, _ptr(pt_src), _ptr(pt_ref), _ptr(idx), _ptr(logits), _ptr(labels),
                                                          _ptr(transform_gt), P, J, K, n, lt, float(wt_ptDist_loss), float(wt_inlier_loss),
                                                          float(loss_discount_factor), _ptr(T), losses, _ptr(grad), pp))
        self.sync()

        def terms(col, zero):
            """The reference's dict for one reduction: col(i, k) = term k of iteration i, zero = 0.0 or zeros [P]."""
            d, total = {}, zero
            for i in range(n):
                disc = loss_discount_factor ** (n - i - 1)
                if wt_ptDist_loss > 0:
                    d[f"{loss_type}_{i}"] = col(i, 0); total = total + disc * d[f"{loss_type}_{i}"]
                else:      # loss.py:793-798: the key stays, at 0
                    d[f"{loss_type}_{i}"] = zero * 0.0
                if wt_inlier_loss > 0 and labels is not None:
                    d[f"outlier_{i}"] = col(i, 1); total = total + disc * d[f"outlier_{i}"]
                if pose:
                    d[f"poseError_{i}"] = col(i, 2); total = total + disc * d[f"poseError_{i}"]
            d["total"] = total
            return d

        out = {"losses": terms(lambda i, k: losses[nc * i + k], 0.0), "grad_logits": grad, "transforms": T}
        if per_pair:      # reduction='none' (loss.py:779, :836): every pair's own terms, [P] each
            a = np.frombuffer(pp, dtype=np.float64).reshape(P, n, nc)
            out["losses_per_pair"] = terms(lambda i, k: a[:, i, k].copy(), np.zeros(P))
        return out

    # ------------------------------------------------------------------ ground-truth matches / inlier targets (include/dsir_train.h)
    def _train_ops(self):
        """The stream-ordered training operators on torch's current stream (deepsir_amd/train.py::_Ops)."""
        from .train import _Ops
        if getattr(self, "_tops", None) is None:
            self._tops = _Ops(self.device)
        self._tops.begin()
        return self._tops

    def radius_matches(self, src, ref, transform_gt, radius: float):
        """The reference loader's get_matching_indices (K = None) for P pairs, brute force on the device: src [P,J,C], ref [P,K,C],
        transform_gt [P,3,4] -> the CSR (offsets [P J + 1] i32, cols [total] i32, ascending per row) of every (j, k) with
        |T_gt src_j - ref_k| < radius.  ``train.as_reference_matches`` turns it into data['matches']."""
        src, ref = _chk(src, torch.float32, "src"), _chk(ref, torch.float32, "ref")
        return self._train_ops().radius_matches(src, ref, _chk(transform_gt, torch.float32, "transform_gt"), radius)

    def match_keys(self, matches: Sequence, hash_seed: int):
        """A batch's match lists (per pair int [n',2] of (src, ref)) hashed and sorted on the device, once per batch."""
        return self._train_ops().match_keys(matches, hash_seed)

    def inlier_targets_matches(self, keys, idx):
        """find_correct_correspondence on the device: idx [n_iter,P,J] i32 -> fp32 0/1 [n_iter,P,J]."""
        return self._train_ops().inlier_targets_matches(keys, _chk(idx, torch.int32, "idx"))

    def inlier_targets_radius(self, src, ref, idx, transform_gt, radius: float):
        """The same targets from geometry alone (the rule of ``radius_matches``): 1 iff |T_gt src_j - ref_idx[j]| < radius."""
        src, ref = _chk(src, torch.float32, "src"), _chk(ref, torch.float32, "ref")
        return self._train_ops().inlier_targets_radius(src, ref, _chk(idx, torch.int32, "idx"), _chk(transform_gt, torch.float32, "transform_gt"),
                                                       radius)

    # ------------------------------------------------------------------ fragment overlap (csrc/overlap.hip; the rule: deepsir_amd/overlap.py)
    def nn_index(self, points, offsets, radius: float, bounds=None):
        """The sparse cell index of F ragged fragments (points [total, C] fp32, offsets [F + 1] on the host), built once; its
        ``search(jobs, poses=None, fill=False)`` runs job lists against it (``train.NNIndex``)."""
        return self._train_ops().nn_index(_chk(points, torch.float32, "points"), offsets, radius, bounds)

    def nn_within(self, points, offsets, jobs, radius: float, poses=None, fill=None, bounds=None):
        """Radius-bounded nearest neighbour of one fragment in another, for a list of jobs: points [total, C] fp32 holding F ragged
        fragments (offsets [F + 1], host), jobs [n, 2] (host) of (query fragment, target fragment), poses None or [n, 3, 4] fp32
        (the query is moved first) -> (counts [n] i32: matched queries per job, nn).  fill: None, or the positions in ``jobs``
        whose neighbour lists are wanted; nn is then a list with one i32 [n_query] tensor per such job (original index in the
        target, or -1).  Raises ValueError with the library's reason, launching nothing, where the call is refused (radius <= 0,
        a job index out of range, an extent of more than 2^21 - 2 cells; the last needs the bounds, which are reduced on the
        device first unless ``bounds`` gives them)."""
        ops = self._train_ops()
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        jobs = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 2))
        why = ops.nn_refusal(off, jobs, radius) if off.size >= 2 else "nn_within: offsets [F + 1] expected"
        if why is not None:
            raise ValueError(why)
        if poses is not None:
            poses = _chk(poses, torch.float32, "poses")
        index = self.nn_index(points, off, radius, bounds)
        counts, _ = index.search(jobs, poses)
        if fill is None:
            return counts, None
        sel = np.asarray(fill, dtype=np.int64).reshape(-1)
        sub = jobs[sel]
        sub_poses = None if poses is None else poses[torch.as_tensor(sel, device=poses.device)].contiguous()
        _, flat = index.search(sub, sub_poses, fill=True)
        rows = index.rows(sub)
        return counts, [flat[rows[k]:rows[k + 1]] for k in range(len(sub))]

    def radius_neighbors(self, points, radius: float, max_nn: int = 0, with_dist: bool = False):
        """The self-neighbourhood of every cloud of a dense batch over the cell index (csrc/radius_nn.hip): points [c, n, C] fp32 ->
        (offsets [c n + 1] i32, cols i32 with cloud-local columns, ascending per row[, d2 fp32 aligned with cols]) - exactly the
        ``csr`` of ``fpfh`` and ``estimate_normals``.  ``max_nn`` = 0: every point within ``radius`` (the bytes of
        ``radius_matches(x, x, identity, radius)``); > 0: the max_nn nearest of them, ties to the lower index (open3d's
        KDTreeSearchParamHybrid).  One fragment and one job (i, i) per cloud.  Raises ValueError where the library refuses the
        call: a bad ``max_nn``, radius, shape or row count before anything is launched, an extent of more than 2^21 - 2 cells after
        the bounds reduction alone."""
        points = _chk(points, torch.float32, "points")
        if points.dim() != 3 or points.shape[2] < 3 or points.shape[0] < 1:
            raise ValueError("radius_neighbors: points [clouds >= 1, n, C >= 3] expected")
        c, n, stride = points.shape
        if int(max_nn) != max_nn or max_nn < 0 or max_nn > 0x7fffffff:
            raise ValueError("nn_radius: max_nn must be 0 (the whole ball) or a positive int32")
        if c * n > (1 << 26) - 1:
            raise ValueError("nn_radius: more than 2^26 - 1 query rows in one job list (one workgroup per row): split it")
        index = self.nn_index(points.reshape(c * n, stride), np.arange(c + 1, dtype=np.int64) * n, radius)
        return index.neighbors(np.repeat(np.arange(c, dtype=np.int32), 2).reshape(c, 2), None, max_nn, with_dist)

    def overlap_ratio(self, src, ref, T, radius: float) -> np.ndarray:
        """The share of every pair's source points that have a reference point within ``radius`` under the pose: src [P, J, C],
        ref [P, K, C], T [P, 3, 4] fp32 -> float64 [P].  The kernels of ``nn_within`` with one job per pair."""
        src, ref, T = _chk(src, torch.float32, "src"), _chk(ref, torch.float32, "ref"), _chk(T, torch.float32, "T")
        P, J, stride = src.shape
        K = ref.shape[1]
        if ref.shape[0] != P or ref.shape[2] != stride or tuple(T.shape) != (P, 3, 4):
            raise ValueError("overlap_ratio: src [P,J,C], ref [P,K,C] and T [P,3,4] expected")
        points = torch.cat([src.reshape(P * J, stride), ref.reshape(P * K, stride)], 0)
        offsets = np.concatenate([np.arange(P + 1, dtype=np.int64) * J, P * J + np.arange(1, P + 1, dtype=np.int64) * K])
        jobs = np.stack([np.arange(P), P + np.arange(P)], 1)
        counts, _ = self.nn_within(points, offsets, jobs, radius, poses=T)
        return counts.cpu().numpy().astype(np.float64) / max(J, 1)

    def enable_graph(self, on=True):
        """Replay dsir_register through a captured hipGraph (same buffers on every call; one graph per call signature)."""
        if on:
            from . import graph_replay_safe
            if not graph_replay_safe():
                raise EngineError("hipGraph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 in the environment BEFORE the process "
                                  "first touches the GPU (this ROCm's graph packet capture replays wrongly; deepsir_amd/__init__.py): "
                                  "import deepsir_amd before creating CUDA tensors, or export the variable")
        self._call(self.lib.dsir_enable_graph(self.h, 1 if on else 0))

    def graph_stats(self) -> Dict[str, int]:
        """Launch census of the registration this engine captured last (include/dsir.h, dsir_graph_stats)."""
        out = (C.c_int64 * 4)()
        self._call(self.lib.dsir_graph_stats(self.h, out))
        return {"nodes": int(out[0]), "kernels": int(out[1]), "memsets": int(out[2]), "memcpys": int(out[3])}

    def enable_walk(self, on=True):
        """A/B switch: the deep pyramid levels of a RandLA pass as one persistent launch (csrc/walk.hip; up to 16 clouds per launch;
        OFF by default - fewer launches, but measured slower) or every layer its own launch.  Same bits either way (include/dsir.h)."""
        self._call(self.lib.dsir_enable_walk(self.h, 1 if on else 0))

    def enable_match_timer(self, on=True):
        self._call(self.lib.dsir_enable_match_timer(self.h, 1 if on else 0))

    def match_timer(self, reset=True):
        ms, n = C.c_double(), C.c_int64()
        self._call(self.lib.dsir_match_timer(self.h, 1 if reset else 0, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def match_timer2(self, reset=True):
        """(operation ms, dominant-kernel ms, launches) of the timed arg-min searches (HIP events on the engine's stream)."""
        op, k, n = C.c_double(), C.c_double(), C.c_int64()
        self._call(self.lib.dsir_match_timer2(self.h, 1 if reset else 0, C.byref(op), C.byref(k), C.byref(n)))
        return op.value, k.value, n.value

    def enable_screen(self, on=True):
        """A/B switch: off = the exhaustive exact-fp32 arg-min kernel throughout (same bits, include/dsir.h)."""
        self._call(self.lib.dsir_enable_screen(self.h, 1 if on else 0))

    def enable_agg_split(self, on=True):
        """A/B switch: fp16-split aggregation chain (default) vs the exact-fp32 chain (include/dsir.h, dsir_enable_agg_split)."""
        self._call(self.lib.dsir_enable_agg_split(self.h, 1 if on else 0))

    SCREEN_STAT_NAMES = ("screened_searches", "rows_searched", "rows_undecided", "pairs_exhaustive", "exhaustive_searches")

    def screen_stats(self, reset=True) -> Dict[str, int]:
        """Which arg-min path dsir_register took since the last reset and how selective the screening was
        (include/dsir.h, dsir_screen_stats)."""
        out = (C.c_int64 * 5)()
        self._call(self.lib.dsir_screen_stats(self.h, 1 if reset else 0, out))
        return {k: int(out[i]) for i, k in enumerate(self.SCREEN_STAT_NAMES)}

    def prune_stats(self, reset=True) -> Tuple[int, int]:
        """(tile products visited, tile products without pruning) of the pruned search since the last reset (dsir_prune_stats)."""
        out = (C.c_int64 * 2)()
        self._call(self.lib.dsir_prune_stats(self.h, 1 if reset else 0, out))
        return int(out[0]), int(out[1])

    def set_prune_thresholds(self, min_points: int = 8192, min_rows: int = 65536):
        """A/B switch: the pruned search runs for ref clouds of min_points points and more (0 = never) in launches of min_rows src
        rows and more; same bits either way (include/dsir.h, dsir_set_prune_thresholds)."""
        self._call(self.lib.dsir_set_prune_thresholds(self.h, int(min_points), int(min_rows)))

    def set_kabsch_chunked_min(self, min_points: int = 0):
        """A/B switch: clouds of min_points points and more solve their pose in chunks (include/dsir.h); <= 0: the default."""
        self._call(self.lib.dsir_set_kabsch_chunked_min(self.h, int(min_points)))

    def match_timer_device(self, reset=True):
        """(total ms, launches) of the timed nn_match launches on the device clock (first wave start .. last wave end)."""
        ms, n = C.c_double(), C.c_int64()
        self._call(self.lib.dsir_match_timer_device(self.h, 1 if reset else 0, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class EnginePool:
    """S engines (each with its own HIP stream and workspace) registering disjoint slices of a batch
    concurrently.  Kernels of one registration are serialised on their stream; two streams let the GPU
    overlap one slice's latency-/memory-bound RandLA kernels with the other's MFMA-bound matching
    (+8-10 % pairs/s on MI355X at 64 pairs, tools/multistream.py).  Results are identical to a single
    engine: pairs are independent and every kernel's tiling depends on the per-cloud shape only."""

    def __init__(self, cfg: NetConfig, device: int = 0, max_points: int = 8192, max_pairs: int = 2, streams: int = 2):
        self.streams = max(1, int(streams))
        self.per = (int(max_pairs) + self.streams - 1) // self.streams
        self.engines = [Engine(cfg, device, max_points, self.per) for _ in range(self.streams)]
        self.cfg, self.device = cfg, self.engines[0].device

    def load_state_dict(self, sd, strict: bool = True):
        for e in self.engines:
            e.load_state_dict(sd, strict)

    def close(self):
        for e in self.engines:
            e.close()

    def sync(self):
        for e in self.engines:
            e.sync()

    def _slices(self, P):
        per = (P + self.streams - 1) // self.streams
        return [(a, min(P, a + per)) for a in range(0, P, per)]

    def register(self, points_src, points_ref, n_iter: int = 5, want_aux: bool = True, sync: bool = True,
                 out: Optional[dict] = None, pyramids: Optional[dict] = None, want_desc: bool = False):
        P = points_src.shape[0]
        if P > self.per * self.streams:
            raise EngineError(f"pairs={P} exceeds the pool's max_pairs={self.per * self.streams}")
        sl = self._slices(P)
        if out is None:
            out = {"transforms": torch.empty((P, n_iter, 3, 4), dtype=torch.float32, device=self.device)}
        parts = []
        for e, (a, b) in zip(self.engines, sl):
            o = {"transforms": out["transforms"][a:b]} if not want_aux else None
            pyr = None if pyramids is None else {k: v[a:b] for k, v in pyramids.items()}
            parts.append(e.register(points_src[a:b], points_ref[a:b], n_iter, want_aux=want_aux, sync=False, out=o,
                                    pyramids=pyr, want_desc=want_desc and want_aux))
        if sync or want_aux:
            self.sync()
        if want_aux:
            out["transforms"] = torch.cat([p["transforms"] for p in parts], 0)
            out["idx"] = torch.cat([p["idx"] for p in parts], 1)
            out["logits"] = torch.cat([p["logits"] for p in parts], 1)
            out["pt_ref_new"] = torch.cat([p["pt_ref_new"] for p in parts], 0)
            out["invalid"] = torch.cat([p["invalid"] for p in parts], 0)
            if want_desc:
                out["desc_src"] = torch.cat([p["desc_src"] for p in parts], 1)
                out["desc_ref"] = torch.cat([p["desc_ref"] for p in parts], 0)
        out["_parts"] = parts
        return out

    def enable_match_timer(self, on=True):
        for e in self.engines:
            e.enable_match_timer(on)

    def match_timer(self, reset=True):
        ms = n = 0
        for e in self.engines:
            m, k = e.match_timer(reset)
            ms, n = ms + m, n + k
        return ms, n

    def match_timer_device(self, reset=True):
        ms = n = 0
        for e in self.engines:
            m, k = e.match_timer_device(reset)
            ms, n = ms + m, n + k
        return ms, n

    def enable_graph(self, on=True):
        for e in self.engines:
            e.enable_graph(on)

    def match_timer2(self, reset=True):
        op = k = n = 0
        for e in self.engines:
            a, b, c = e.match_timer2(reset)
            op, k, n = op + a, k + b, n + c
        return op, k, n

    def enable_screen(self, on=True):
        for e in self.engines:
            e.enable_screen(on)

    def enable_agg_split(self, on=True):
        for e in self.engines:
            e.enable_agg_split(on)

    def screen_stats(self, reset=True) -> Dict[str, int]:
        tot: Dict[str, int] = {}
        for e in self.engines:
            for k, v in e.screen_stats(reset).items():
                tot[k] = tot.get(k, 0) + v
        return tot
