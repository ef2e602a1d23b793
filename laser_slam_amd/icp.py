"""Host-side mirror of the ICP object seam the reference calls (seam B2).

The reference owns a ``PointMatcher::ICP icp_`` (laser_slam/include/laser_slam/laser_track.hpp:217,
incremental_estimator.hpp:70) and uses exactly three members of it:

    icp_.loadFromYaml(std::istream&)      laser_slam/src/laser_track.cpp:17
    icp_.setDefault()                     laser_slam/src/laser_track.cpp:20
    icp_.compute(reading, reference, T)   laser_slam/src/laser_track.cpp:496,
                                          laser_slam/src/incremental_estimator.cpp:108

``ICP`` below keeps those names/semantics (snake_case) over the C ABI in include/lsgpu_icp.h;
``IcpHandle`` is the thin 1:1 wrapper of that ABI.  Clouds are (N,4) float32 x,y,z,1 arrays
(DataPoints.features transposed: memory is identical to Eigen's column-major 4xN); they may be numpy
arrays (host) or torch CUDA tensors (HBM-resident, zero copy).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib
from ._lib import ConvergenceError, IcpConfig, IcpStats, IterTrace, LsgpuError

try:  # torch is plumbing only (device memory); the package works without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _as_f32(x, cols: int):
    """-> (address, keepalive, n_rows).  numpy: C-contiguous float32 copy if needed."""
    if _is_torch(x):
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != cols:
            raise ValueError(f"expected (N,{cols}) tensor, got {tuple(x.shape)}")
        if x.is_cuda:
            # stream contract of include/lsgpu_icp.h: the library works on the handle's own (non-blocking) stream, so
            # whatever torch still has in flight for this tensor -- including the copy made just above -- must be done
            torch.cuda.current_stream(x.device).synchronize()
        return (x.data_ptr() if x.numel() else None), x, x.shape[0]
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"expected (N,{cols}) array, got {a.shape}")
    return (a.ctypes.data if a.size else None), a, a.shape[0]


def _t16(T) -> np.ndarray:
    """4x4 (row-major numpy) or 16 column-major floats -> 16 float32 column-major."""
    T = np.asarray(T)
    if T.shape == (4, 4):
        return np.ascontiguousarray(T.astype(np.float32).T).reshape(16)
    if T.size == 16:
        return np.ascontiguousarray(T, np.float32).reshape(16)
    raise ValueError("transform must be 4x4 or 16 floats")


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _raise(code: int, what: str, h=None):
    detail = ""
    if h is not None:
        detail = _lib.lib().lsgpu_last_error(h).decode()
    if code == _lib.NO_CONVERGENCE:
        raise ConvergenceError(code, what, detail)
    raise LsgpuError(code, what, detail)


class IcpHandle:
    """One lsgpu_icp handle == one reference ``icp_`` member: one device, one HIP stream."""

    def __init__(self, cfg: Optional[IcpConfig] = None, device: int = 0, error_minimizer=None, matcher_knn=None,
                 matcher_max_dist=None, outlier_max_dist=None, outlier_min_dist=None, outlier_median_factor=None,
                 robust=None, normals=None, covariance=None, cuts=None, max_density=None, shadow=None, motion=None,
                 cov_sampling=None):
        """error_minimizer: None (cfg's), a module name ("PointToPlaneErrorMinimizer" / "PointToPointErrorMinimizer")
        or an _lib.MINIMIZER_* value.  matcher_knn: None (cfg's) or KDTreeMatcher's knn, 1.._lib.MATCHER_KNN_MAX (k >= 2:
        every reading point is paired with its k nearest reference points).  matcher_max_dist: KDTreeMatcher's maxDist;
        outlier_max_dist / outlier_min_dist / outlier_median_factor: Max- / Min- / MedianDistOutlierFilter's parameter
        (None: cfg's; 0: no such module; see lsgpu_icp_config).  robust: None, or RobustOutlierFilter's parameters (a
        RobustConfig, a dict of its fields, or an _lib.RobustCfg) -- lsgpu_icp_set_robust_filter.  normals: None, or a
        NormalsConfig / dict of its fields / _lib.NormalsCfg (SurfaceNormalOutlierFilter, reading normals, oriented
        normals) -- lsgpu_icp_set_normals.  covariance: None, or PointToPlaneWithCovErrorMinimizer's sensorStdDev --
        lsgpu_icp_set_covariance.  cuts: None, or the
        cut modules of the two filter sections (a ChainCuts, a dict of its fields, or an _lib.ChainCuts) --
        lsgpu_icp_set_chain_cuts.  max_density: None, or MaxDensityDataPointsFilter's maxDensity behind the reference's
        SurfaceNormalDataPointsFilter (compute's sn_knn) -- lsgpu_icp_set_max_density.  shadow: None, or
        ShadowDataPointsFilter's eps as (reading_eps, reference_eps), None or a negative value for a side without the module
        (a dict with those keys or an _lib.ShadowCfg too) -- lsgpu_icp_set_shadow (the reading's needs `normals` with
        reading_sn_knn).  motion: None, or PointToPlaneErrorMinimizer's force2D / force4DOF and BoundTransformationChecker (a
        MotionConfig, a dict of its fields, or an _lib.MotionCfg) -- lsgpu_icp_set_motion.  cov_sampling: None, or CovarianceSamplingDataPointsFilter's
        ((reading_nb_sample, reading_torque_norm), (reference_nb_sample, reference_torque_norm)), None for a side without the
        module (a dict of lsgpu_cov_sampling_config's fields or an _lib.CovSamplingCfg too) -- lsgpu_icp_set_cov_sampling (the
        reading's needs `normals` with reading_sn_knn).  The modules are applied together (lsgpu_icp_set_modules): which of them
        go together is the library's rule set, and a refusal leaves no handle behind."""
        L = _lib.lib()
        nc = normals_cfg(normals) if normals is not None else None
        if nc is not None:                                      # refused values: before the device is touched
            why = L.lsgpu_normals_config_why(C.byref(nc), 0, 1)
            if why:
                raise LsgpuError(_lib.BAD_CONFIG, "lsgpu_normals_config_check", why.decode())
        rb = robust_cfg(robust) if robust is not None else None
        if rb is not None:                                      # refused values: before the device is touched
            mini = _MINIMIZERS.get(error_minimizer, error_minimizer) if error_minimizer is not None else (cfg.error_minimizer if cfg is not None else 0)
            why = L.lsgpu_robust_config_why(C.byref(rb), int(mini), 1)
            if why:
                raise LsgpuError(_lib.BAD_CONFIG, "lsgpu_robust_config_check", why.decode())
        if cfg is None:
            cfg = IcpConfig()
            L.lsgpu_icp_config_yaml(C.byref(cfg))
        thresholds = {"matcher_max_dist": matcher_max_dist, "outlier_max_dist": outlier_max_dist,
                      "outlier_min_dist": outlier_min_dist, "outlier_median_factor": outlier_median_factor}
        if error_minimizer is not None or matcher_knn is not None or any(v is not None for v in thresholds.values()):
            cfg = IcpConfig.from_buffer_copy(cfg)       # (the caller's config stays as it is)
            for name, v in thresholds.items():
                if v is not None:
                    setattr(cfg, name, float(v))
            if error_minimizer is not None:
                cfg.error_minimizer = _MINIMIZERS.get(error_minimizer, error_minimizer)
            if matcher_knn is not None:
                cfg.matcher_knn = int(matcher_knn)
        self.cfg = cfg
        self.device = device
        self._h = C.c_void_p()
        rc = L.lsgpu_icp_create(C.byref(cfg), device, C.byref(self._h))
        if rc != _lib.OK:
            self._h = None
            _raise(rc, "lsgpu_icp_create (is a ROCm GPU visible?)")
        # the module set as one record (what lsgpu_chain_load_modules makes of a document), applied in one call: all or nothing
        m = _lib.ChainModules()
        for default, part in ((L.lsgpu_shadow_config_default, m.shadow), (L.lsgpu_motion_config_default, m.motion),
                              (L.lsgpu_cov_sampling_config_default, m.cov_sampling)):
            default(C.byref(part))
        if rb is not None:
            m.chain.robust, m.chain.has_robust = rb, 1
        if nc is not None:
            m.chain.normals, m.chain.has_normals = nc, 1
        # (the two values lsgpu_loaded_chain carries in reserved[]: flag and float, as lsgpu_loaded_chain_covariance / _max_density read them)
        for at, v in ((0, covariance), (4, max_density)):
            if v is not None:
                m.chain.reserved[at] = 1
                m.chain.reserved[at + 1] = int(np.float32(v).view(np.int32))
        if cuts is not None:
            m.cuts = chain_cuts_cfg(cuts)
        if shadow is not None:
            m.shadow = shadow_cfg(shadow)
        if cov_sampling is not None:
            m.cov_sampling = cov_sampling_cfg(cov_sampling)
        if motion is not None:
            m.motion = motion_cfg(motion)
        rc = L.lsgpu_icp_set_modules(self._h, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_modules", self._h)
        self.robust, self.normals = rb, nc
        self.covariance = None if covariance is None else float(np.float32(covariance))
        self.cuts = m.cuts if m.cuts.n_reading or m.cuts.n_reference else None
        self.max_density = None if max_density is None else float(np.float32(max_density))
        self.shadow = (float(m.shadow.reading_eps), float(m.shadow.reference_eps)) if m.shadow.reading_eps >= 0 or m.shadow.reference_eps >= 0 else None
        self.cov_sampling = _cov_sampling_pairs(m.cov_sampling) if cov_sampling is not None else None
        self.motion = _motion_config(m.motion) if m.motion.dof or m.motion.bound else None

    def set_motion(self, motion):
        """lsgpu_icp_set_motion: PointToPlaneErrorMinimizer's force2D / force4DOF step and BoundTransformationChecker of this
        handle's alignments.  motion: a MotionConfig, a dict of its fields or an _lib.MotionCfg; None: off."""
        mc = motion_cfg(motion) if motion is not None else None
        rc = _lib.lib().lsgpu_icp_set_motion(self._h, C.byref(mc) if mc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_motion", self._h)
        self.motion = _motion_config(mc) if mc is not None and (mc.dof or mc.bound) else None

    def set_cov_sampling(self, cov_sampling):
        """lsgpu_icp_set_cov_sampling: CovarianceSamplingDataPointsFilter as the last thinning step of the reading's / the
        reference's section of this handle's compute calls.  cov_sampling: ((reading_nb_sample, reading_torque_norm),
        (reference_nb_sample, reference_torque_norm)) with None for a side without the module, a dict of
        lsgpu_cov_sampling_config's fields or an _lib.CovSamplingCfg; None: off."""
        cc = cov_sampling_cfg(cov_sampling) if cov_sampling is not None else None
        rc = _lib.lib().lsgpu_icp_set_cov_sampling(self._h, C.byref(cc) if cc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_cov_sampling", self._h)
        self.cov_sampling = _cov_sampling_pairs(cc) if cc is not None else None

    def set_shadow(self, shadow):
        """lsgpu_icp_set_shadow: ShadowDataPointsFilter behind the normals of the reading's / the reference's section of this
        handle's compute calls.  shadow: (reading_eps, reference_eps), a dict with those keys or an _lib.ShadowCfg; None or a
        negative eps: no module on that side; None: off."""
        sc = shadow_cfg(shadow) if shadow is not None else None
        rc = _lib.lib().lsgpu_icp_set_shadow(self._h, C.byref(sc) if sc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_shadow", self._h)
        on = sc is not None and (sc.reading_eps >= 0 or sc.reference_eps >= 0)
        self.shadow = (float(sc.reading_eps), float(sc.reference_eps)) if on else None

    def filter_shadow(self, xyz1, normals, eps: float = 0.1):
        """ShadowDataPointsFilter on the GPU (lsgpu_icp_filter_shadow) -> (xyz1', normals').  torch CUDA inputs give torch CUDA
        outputs, anything else numpy.  Raises ConvergenceError if nothing is kept."""
        p, _k, n = _as_f32(xyz1, 4)
        q, _k3, m = _as_f32(normals, 3)
        if m != n:
            raise ValueError(f"{n} points, {m} normals")
        if _is_torch(xyz1) and xyz1.is_cuda and _is_torch(normals) and normals.is_cuda:
            o = torch.empty((max(n, 1), 4), dtype=torch.float32, device=xyz1.device)
            nr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz1.device)
            torch.cuda.synchronize()
            po, pn = o.data_ptr(), nr.data_ptr()
        else:
            o = np.empty((max(n, 1), 4), np.float32)
            nr = np.empty((max(n, 1), 3), np.float32)
            po, pn = o.ctypes.data, nr.ctypes.data
        k = C.c_int64(0)
        rc = _lib.lib().lsgpu_icp_filter_shadow(self._h, p, q, n, float(eps), po, pn, C.byref(k))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_shadow", self._h)
        return o[:k.value], nr[:k.value]

    def filter_cov_sampling(self, xyz1, normals, nb_sample: int = 5000, torque_norm: int = 1, return_sums: bool = False):
        """CovarianceSamplingDataPointsFilter on the GPU (lsgpu_icp_filter_cov_sampling) -> (xyz1', normals', ids) in pick
        order, with return_sums also the 32 sums the device formed (numpy float64).  torch CUDA inputs give torch CUDA outputs
        (ids int32), anything else numpy."""
        p, _k, n = _as_f32(xyz1, 4)
        q, _k3, m = _as_f32(normals, 3)
        if m != n:
            raise ValueError(f"{n} points, {m} normals")
        nb = _c_int(nb_sample)
        room = max(min(nb, n), 1)
        if _is_torch(xyz1) and xyz1.is_cuda and _is_torch(normals) and normals.is_cuda:
            o = torch.empty((room, 4), dtype=torch.float32, device=xyz1.device)
            nr = torch.empty((room, 3), dtype=torch.float32, device=xyz1.device)
            ids = torch.empty((room,), dtype=torch.int32, device=xyz1.device)
            torch.cuda.synchronize()
            po, pn, pi = o.data_ptr(), nr.data_ptr(), ids.data_ptr()
        else:
            o = np.empty((room, 4), np.float32)
            nr = np.empty((room, 3), np.float32)
            ids = np.empty((room,), np.int32)
            po, pn, pi = o.ctypes.data, nr.ctypes.data, ids.ctypes.data
        sums = np.zeros(32, np.float64)
        k = C.c_int64(0)
        rc = _lib.lib().lsgpu_icp_filter_cov_sampling(self._h, p, q, n, nb, _c_int(torque_norm), po, pn, pi, C.byref(k),
                                                      sums.ctypes.data)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_cov_sampling", self._h)
        out = (o[:k.value], nr[:k.value], ids[:k.value])
        return out + (sums,) if return_sums else out

    def cov_sampling_phase_ms(self):
        """Wall time in ms of the four phases of this handle's last filter_cov_sampling (lsgpu_icp_cov_sampling_phase_ms):
        sums, projections + sorts + heads download, host walk, picks upload + gather (enqueue)."""
        ms = (C.c_double * 4)()
        rc = _lib.lib().lsgpu_icp_cov_sampling_phase_ms(self._h, ms)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_cov_sampling_phase_ms", self._h)
        return [float(x) for x in ms]

    def set_max_density(self, max_density=10.0):
        """lsgpu_icp_set_max_density: MaxDensityDataPointsFilter behind SurfaceNormalDataPointsFilter keepDensities 1 in the
        reference section of this handle's compute calls (None: off)."""
        mc = None
        if max_density is not None:
            mc = _lib.MaxDensityCfg()
            _lib.lib().lsgpu_max_density_config_default(C.byref(mc))
            mc.max_density = float(max_density)
        rc = _lib.lib().lsgpu_icp_set_max_density(self._h, C.byref(mc) if mc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_max_density", self._h)
        self.max_density = None if mc is None else float(mc.max_density)

    def filter_reference_max_density(self, xyz1, knn: int = 10, max_density: float = 10.0, seed: int = -1,
                                     with_densities: bool = False):
        """SurfaceNormalDataPointsFilter keepDensities 1 + MaxDensityDataPointsFilter on the GPU
        (lsgpu_icp_filter_reference_max_density) -> (xyz1', normals, n_dense), or (xyz1', normals, n_dense, densities of the
        INPUT points) with `with_densities`.  torch CUDA input gives torch CUDA output, anything else numpy."""
        p, _k, n = _as_f32(xyz1, 4)
        knn = int(knn)
        if not 3 <= knn <= 32:
            raise LsgpuError(_lib.BAD_ARG, "lsgpu_icp_filter_reference_max_density", "knn must be in [3, 32]")
        if _is_torch(xyz1) and xyz1.is_cuda:
            o = torch.empty((max(n, 1), 4), dtype=torch.float32, device=xyz1.device)
            nr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz1.device)
            dn = torch.empty((max(n, 1),), dtype=torch.float32, device=xyz1.device) if with_densities else None
            torch.cuda.synchronize()
            po, pn, pd = o.data_ptr(), nr.data_ptr(), (dn.data_ptr() if with_densities else None)
        else:
            o = np.empty((max(n, 1), 4), np.float32)
            nr = np.empty((max(n, 1), 3), np.float32)
            dn = np.empty((max(n, 1),), np.float32) if with_densities else None
            po, pn, pd = o.ctypes.data, nr.ctypes.data, (dn.ctypes.data if with_densities else None)
        m, nd = C.c_int64(0), C.c_int64(0)
        rc = _lib.lib().lsgpu_icp_filter_reference_max_density(self._h, p, n, knn, float(max_density), seed, po, pn, pd,
                                                               C.byref(m), C.byref(nd))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_reference_max_density", self._h)
        return (o[:m.value], nr[:m.value], nd.value, dn[:n]) if with_densities else (o[:m.value], nr[:m.value], nd.value)

    def set_chain_cuts(self, cuts):
        """lsgpu_icp_set_chain_cuts: MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter in the filter sections of
        this handle's compute calls (None, or no module at all, switches them off)."""
        cc = chain_cuts_cfg(cuts) if cuts is not None else None
        rc = _lib.lib().lsgpu_icp_set_chain_cuts(self._h, C.byref(cc) if cc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_chain_cuts", self._h)
        self.cuts = cc if cc is not None and (cc.n_reading or cc.n_reference) else None

    def filter_section(self, cuts, side: int, xyz1, prob: float = -1.0, seed: int = -1):
        """lsgpu_icp_filter_section: the fused pass of one filter section alone -> xyz1'.  side 0: the reading's cut modules
        with RandomSampling of probability `prob` at cuts.reading_sampling_at (prob < 0: none); side 1: the reference's."""
        cc = chain_cuts_cfg(cuts)
        p, _k, n = _as_f32(xyz1, 4)
        o, po = self._filter_out(xyz1, n)
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_icp_filter_section(self._h, C.byref(cc), int(side), float(prob), p, n, seed, po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_section", self._h)
        return o[:m.value]

    def set_covariance(self, sensor_std_dev=0.01):
        """lsgpu_icp_set_covariance: PointToPlaneWithCovErrorMinimizer's covariance after every alignment (None: off)."""
        cc = None
        if sensor_std_dev is not None:
            cc = _lib.CovarianceCfg()
            _lib.lib().lsgpu_covariance_config_default(C.byref(cc))
            cc.sensor_std_dev = float(sensor_std_dev)
        rc = _lib.lib().lsgpu_icp_set_covariance(self._h, C.byref(cc) if cc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_covariance", self._h)
        self.covariance = None if cc is None else float(cc.sensor_std_dev)

    def quality(self):
        """lsgpu_icp_get_quality of the last alignment -> dict(covariance 6x6 float64, residual, n_pairs, used_ratio).
        Raises LsgpuError (BAD_CONFIG: covariance off) / ConvergenceError (no OK alignment yet, singular H)."""
        q = _lib.IcpQuality()
        rc = _lib.lib().lsgpu_icp_get_quality(self._h, C.byref(q))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_get_quality", self._h)
        return dict(covariance=np.array(q.covariance[:], np.float64).reshape(6, 6), residual=float(q.residual),
                    n_pairs=int(q.n_pairs), used_ratio=float(q.used_ratio))

    def point_to_plane_cov(self, query_xyz1, T, ids, d2, limit: float, dT=None) -> np.ndarray:
        """lsgpu_point_to_plane_cov: the 44 covariance sums (21 of H, 21 of M, count, sum (n . (p - q))^2) of the pairs
        with d2 <= limit under the step dT (4x4; None: identity), double."""
        p, _k, n = _as_f32(query_xyz1, 4)
        ids = np.ascontiguousarray(ids, np.int32)
        d2 = np.ascontiguousarray(d2, np.float32)
        out = np.zeros(44)
        tp = _fp(_t16(T)) if T is not None else None
        dp = _fp(_t16(dT)) if dT is not None else None
        rc = _lib.lib().lsgpu_point_to_plane_cov(self._h, p, n, tp, ids.ctypes.data, d2.ctypes.data, limit, dp,
                                                 out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_point_to_plane_cov", self._h)
        return out

    def set_normals(self, normals):
        """lsgpu_icp_set_normals: SurfaceNormalOutlierFilter / reading normals / oriented normals (None removes them)."""
        nc = normals_cfg(normals) if normals is not None else None
        rc = _lib.lib().lsgpu_icp_set_normals(self._h, C.byref(nc) if nc is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_normals", self._h)
        self.normals = nc

    def reads_reference_normals(self) -> bool:
        """Does a module behind the reference's section read its normals: a minimizer other than point-to-point,
        RobustOutlierFilter with the point-to-plane distance, or SurfaceNormalOutlierFilter."""
        return (self.cfg.error_minimizer != _lib.MINIMIZER_POINT_TO_POINT
                or (self.robust is not None and self.robust.distance_type == _lib.ROBUST_DIST["point2plane"])
                or (self.normals is not None and self.normals.max_angle >= 0))

    def normal_angle_trace(self, cap: int = 64):
        """lsgpu_icp_get_normal_angle_trace: per iteration of the last align {rejected, eps}."""
        buf = (_lib.NormalAngleTrace * cap)()
        n = _lib.lib().lsgpu_icp_get_normal_angle_trace(self._h, buf, cap)
        return [dict(rejected=int(buf[i].rejected), eps=np.float32(buf[i].eps)) for i in range(n)]

    def reading_normals(self, xyz1, knn: int = 5, orient: int = 0, sensor=(0.0, 0.0, 0.0)) -> np.ndarray:
        """lsgpu_icp_reading_normals: SurfaceNormalDataPointsFilter on a reading (+ orientation); the handle's reference stays."""
        p, _k, n = _as_f32(xyz1, 4)
        out = np.empty((n, 3), np.float32)
        sv = np.asarray(sensor, np.float32)
        rc = _lib.lib().lsgpu_icp_reading_normals(self._h, p, n, int(knn), int(orient), _fp(sv), out.ctypes.data)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_reading_normals", self._h)
        return out

    def reference_normals(self) -> np.ndarray:
        """lsgpu_icp_get_reference_normals: the handle's reference normals in the order the reference was given."""
        n = int(self.info().n_reference)
        out = np.empty((n, 3), np.float32)
        rc = _lib.lib().lsgpu_icp_get_reference_normals(self._h, out.ctypes.data, n)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_get_reference_normals", self._h)
        return out

    def align_normals(self, reading_xyz1, reading_normals, T_init):
        """lsgpu_icp_align_normals: align with the reading's normals (n x 3) -> (T 4x4 float32, IcpStats)."""
        p, _k, n = _as_f32(reading_xyz1, 4)
        q, _k2, m = _as_f32(reading_normals, 3)
        if m != n:
            raise ValueError("normals must have one row per reading point")
        ti = _t16(T_init)
        to = np.empty(16, np.float32)
        st = IcpStats()
        rc = _lib.lib().lsgpu_icp_align_normals(self._h, p, n, q, _fp(ti), _fp(to), C.byref(st))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_align_normals", self._h)
        return to.reshape(4, 4).T.copy(), st

    def set_robust_filter(self, robust):
        """lsgpu_icp_set_robust_filter: RobustOutlierFilter on this handle (None removes it)."""
        rb = robust_cfg(robust) if robust is not None else None
        rc = _lib.lib().lsgpu_icp_set_robust_filter(self._h, C.byref(rb) if rb is not None else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_robust_filter", self._h)
        self.robust = rb

    def robust_trace(self, cap: int = 64):
        """lsgpu_icp_get_robust_trace: per iteration of the last align {median, scale, w_sum, recomputed}."""
        buf = (_lib.RobustTrace * cap)()
        n = _lib.lib().lsgpu_icp_get_robust_trace(self._h, buf, cap)
        return [dict(median=np.float32(buf[i].median), scale=np.float32(buf[i].scale), w_sum=float(buf[i].w_sum),
                     recomputed=int(buf[i].recomputed)) for i in range(n)]

    def close(self):
        if getattr(self, "_h", None) and _lib is not None and _lib._lib is not None:
            _lib._lib.lsgpu_icp_destroy(self._h)  # (module globals may be gone at interpreter exit)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- ICP::compute steps 2-3
    def set_reference(self, ref_xyz1, ref_normals=None):
        """ref_normals None: no normals (a point-to-point handle reads none)."""
        p, _k1, n = _as_f32(ref_xyz1, 4)
        q, _k2, m = _as_f32(ref_normals, 3) if ref_normals is not None else (None, None, n)
        if m != n:
            raise ValueError("normals must have one row per reference point")
        rc = _lib.lib().lsgpu_icp_set_reference(self._h, p, q, n)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_set_reference", self._h)

    def reference_mean(self) -> np.ndarray:
        m = np.zeros(3, np.float32)
        rc = _lib.lib().lsgpu_icp_get_reference_mean(self._h, _fp(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_get_reference_mean", self._h)
        return m

    def comm_init(self, rank: int, nranks: int, unique_id: bytes):
        """Split-scan mode: this handle's align() now takes the LOCAL shard of the reading and
        all-reduces the select histograms and normal-equation sums over RCCL (include/lsgpu_icp.h)."""
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        rc = _lib.lib().lsgpu_icp_comm_init(self._h, rank, nranks, unique_id)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_comm_init", self._h)

    def info(self) -> "_lib.IcpInfo":
        out = _lib.IcpInfo()
        rc = _lib.lib().lsgpu_icp_get_info(self._h, C.byref(out))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_get_info", self._h)
        return out

    def policy_info(self):
        """lsgpu_icp_get_policy_info: what the handle's launch policy remembers across calls (index rest, fallbacks)."""
        out = _lib.PolicyInfo()
        rc = _lib.lib().lsgpu_icp_get_policy_info(self._h, C.byref(out))
        if rc:
            _raise(rc, "lsgpu_icp_get_policy_info", self._h)
        return out

    # ---- ICP::compute steps 5-7
    def align(self, reading_xyz1, T_init):
        """-> (T 4x4 float32, IcpStats).  Raises ConvergenceError like PointMatcher."""
        p, _k, n = _as_f32(reading_xyz1, 4)
        ti = _t16(T_init)
        to = np.empty(16, np.float32)
        st = IcpStats()
        rc = _lib.lib().lsgpu_icp_align(self._h, p, n, _fp(ti), _fp(to), C.byref(st))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_align", self._h)
        return to.reshape(4, 4).T.copy(), st

    # ---- the sampling filters on the device, and the whole of ICP::compute
    def filter_reference(self, xyz1, knn: int = 10, ratio: float = 0.5, seed: int = -1):
        """SamplingSurfaceNormalDataPointsFilter (icp_default.yaml:5-7) on the GPU -> (xyz1', normals);
        torch CUDA input gives torch CUDA output, anything else numpy."""
        p, _k, n = _as_f32(xyz1, 4)
        m = C.c_int64(0)
        if _is_torch(xyz1) and xyz1.is_cuda:
            o = torch.empty((max(n, 1), 4), dtype=torch.float32, device=xyz1.device)
            nr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz1.device)
            torch.cuda.synchronize()
            po, pn = o.data_ptr(), nr.data_ptr()
        else:
            o = np.empty((max(n, 1), 4), np.float32)
            nr = np.empty((max(n, 1), 3), np.float32)
            po, pn = o.ctypes.data, nr.ctypes.data
        rc = _lib.lib().lsgpu_icp_filter_reference(self._h, p, n, knn, ratio, seed, po, pn, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_reference", self._h)
        return o[:m.value], nr[:m.value]

    def filter_reference_normals(self, xyz1, knn: int = 5, with_neighbours: bool = False, with_densities: bool = False):
        """SurfaceNormalDataPointsFilter on the GPU: every point keeps its place and gets the PCA normal of its knn
        nearest neighbours, itself included (include/lsgpu_icp.h has the contract) -> normals (n, 3), or
        (normals, ids (n, knn) int32, d2 (n, knn)) with `with_neighbours`.  torch CUDA input gives torch CUDA output,
        anything else numpy.  The cloud becomes the handle's reference, with these normals.  with_densities (keepDensities
        1): the density of every point, (n,), is appended to the result."""
        p, _k, n = _as_f32(xyz1, 4)
        knn = int(knn)
        if not 3 <= knn <= 32:                                   # (before any output is sized with it)
            raise LsgpuError(_lib.BAD_ARG, "lsgpu_icp_filter_reference_normals", "knn must be in [3, 32]")
        dev = _is_torch(xyz1) and xyz1.is_cuda
        if dev:
            nr = torch.empty((max(n, 1), 3), dtype=torch.float32, device=xyz1.device)
            ids = torch.empty((max(n, 1), knn), dtype=torch.int32, device=xyz1.device) if with_neighbours else None
            d2 = torch.empty((max(n, 1), knn), dtype=torch.float32, device=xyz1.device) if with_neighbours else None
            torch.cuda.synchronize()
            dn = torch.empty((max(n, 1),), dtype=torch.float32, device=xyz1.device) if with_densities else None
            pn, pi, pd = nr.data_ptr(), (ids.data_ptr() if with_neighbours else None), (d2.data_ptr() if with_neighbours else None)
            pdn = dn.data_ptr() if with_densities else None
        else:
            nr = np.empty((max(n, 1), 3), np.float32)
            ids = np.empty((max(n, 1), knn), np.int32) if with_neighbours else None
            d2 = np.empty((max(n, 1), knn), np.float32) if with_neighbours else None
            dn = np.empty((max(n, 1),), np.float32) if with_densities else None
            pn, pi, pd = nr.ctypes.data, (ids.ctypes.data if with_neighbours else None), (d2.ctypes.data if with_neighbours else None)
            pdn = dn.ctypes.data if with_densities else None
        if with_densities:
            rc = _lib.lib().lsgpu_icp_filter_reference_normals_densities(self._h, p, n, int(knn), pn, pi, pd, pdn)
        else:
            rc = _lib.lib().lsgpu_icp_filter_reference_normals(self._h, p, n, int(knn), pn, pi, pd)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_reference_normals", self._h)
        out = (nr[:n], ids[:n], d2[:n]) if with_neighbours else (nr[:n],)
        if with_densities:
            out += (dn[:n],)
        return out if len(out) > 1 else out[0]

    def filter_reading(self, xyz1, prob: float = 0.5, seed: int = -1):
        """RandomSamplingDataPointsFilter (icp_default.yaml:1-3) on the GPU -> xyz1'."""
        p, _k, n = _as_f32(xyz1, 4)
        m = C.c_int64(0)
        if _is_torch(xyz1) and xyz1.is_cuda:
            o = torch.empty((max(n, 1), 4), dtype=torch.float32, device=xyz1.device)
            torch.cuda.synchronize()
            po = o.data_ptr()
        else:
            o = np.empty((max(n, 1), 4), np.float32)
            po = o.ctypes.data
        rc = _lib.lib().lsgpu_icp_filter_reading(self._h, p, n, prob, seed, po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_filter_reading", self._h)
        return o[:m.value]

    def compute(self, reading_xyz1, reference_xyz1, T_init, reading_prob: float = 0.5, ssn_knn: int = 10,
                ssn_ratio: float = 0.5, seed: int = -1, sn_knn: int = 0, reading_normals=None, reference_normals=None):
        """``icp_.compute(reading, reference, T_init)`` entirely on the device: reference filter,
        set_reference, reading filter, align.  -> (T 4x4, IcpStats); raises ConvergenceError.
        sn_knn > 0 (with ssn_knn 0): SurfaceNormalDataPointsFilter is the reference filter.
        reading_normals / reference_normals: the normals the clouds carry, (N, 3) beside the points
        (lsgpu_icp_compute_normals; include/lsgpu_icp.h, "carried normals")."""
        q, _k1, nq = _as_f32(reading_xyz1, 4)
        r, _k2, nr = _as_f32(reference_xyz1, 4)
        ch = _lib.ChainCfg(reading_prob, ssn_knn, ssn_ratio, int(sn_knn), seed)
        ti = _t16(T_init)
        to = np.empty(16, np.float32)
        st = IcpStats()
        if reading_normals is None and reference_normals is None:
            rc = _lib.lib().lsgpu_icp_compute(self._h, q, nq, r, nr, _fp(ti), C.byref(ch), _fp(to), C.byref(st))
            if rc != _lib.OK:
                _raise(rc, "lsgpu_icp_compute", self._h)
            return to.reshape(4, 4).T.copy(), st
        qn, _k3 = self._carried(reading_normals, nq, "reading_normals")
        rn, _k4 = self._carried(reference_normals, nr, "reference_normals")
        rc = _lib.lib().lsgpu_icp_compute_normals(self._h, q, qn, nq, r, rn, nr, _fp(ti), C.byref(ch), _fp(to), C.byref(st))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_compute_normals", self._h)
        return to.reshape(4, 4).T.copy(), st

    @staticmethod
    def _carried(normals, n: int, what: str):
        """-> (address or None, keepalive) of the (n, 3) normals a cloud of n points carries.  An empty cloud's normals are
        handed over by a valid address all the same: NULL means "carries none"."""
        if normals is None:
            return None, None
        p, keep, m = _as_f32(normals, 3)
        if m != n:
            raise ValueError(f"{what}: {m} normals for {n} points")
        if p is None:
            keep = np.zeros((1, 3), np.float32)
            p = keep.ctypes.data
        return p, keep

    # ---- local-map maintenance (laser_slam_ros worker): cylinder crop, voxel grid
    def _filter_out(self, xyz1, n):
        if _is_torch(xyz1) and xyz1.is_cuda:
            o = torch.empty((max(n, 1), 4), dtype=torch.float32, device=xyz1.device)
            torch.cuda.synchronize()
            return o, o.data_ptr()
        o = np.empty((max(n, 1), 4), np.float32)
        return o, o.ctypes.data

    def filter_cylinder(self, xyz1, center, radius_m: float, height_m: float, remove_point_inside: bool = False):
        """applyCylindricalFilter (laser_slam_ros common.hpp:194-223) on the GPU, order preserved."""
        p, _k, n = _as_f32(xyz1, 4)
        c = np.ascontiguousarray(center, np.float32).reshape(3)
        o, po = self._filter_out(xyz1, n)
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_filter_cylinder(self._h, p, n, _fp(c), radius_m, height_m, int(remove_point_inside),
                                              po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_filter_cylinder", self._h)
        return o[:m.value]

    def filter_voxel_grid(self, xyz1, leaf, min_points: int = 1):
        """pcl::VoxelGrid (laser_slam_worker.cpp:70-72, 439-440) on the GPU: one centroid per occupied voxel."""
        p, _k, n = _as_f32(xyz1, 4)
        lf = np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float32), (3,)), np.float32)
        o, po = self._filter_out(xyz1, n)
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_filter_voxel_grid(self._h, p, n, _fp(lf), int(min_points), po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_filter_voxel_grid", self._h)
        return o[:m.value]

    # ---- the input filter chain (laser_track.cpp:24-30, :146)
    def apply_point_filters(self, filters, xyz1, seed: int = -1):
        """`filters`: ctypes array of _lib.PointFilter (FixStepSampling's `state` is updated in place)."""
        p, _k, n = _as_f32(xyz1, 4)
        o, po = self._filter_out(xyz1, n)
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_apply_point_filters(self._h, filters, len(filters), p, n, seed, po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_apply_point_filters", self._h)
        return o[:m.value]

    # ---- ROS message surface: sensor_msgs/PointCloud2 data block <-> x,y,z,1 (laser_slam_worker.cpp:125, common.hpp:159-191)
    def cloud_from_pointcloud2(self, data, n_points: int, point_step: int, off_x: int, off_y: int, off_z: int,
                               is_bigendian: bool = False, is_dense: bool = True, device_out: bool = False):
        """`data`: bytes / uint8 numpy array / uint8 torch tensor holding n_points records of point_step bytes."""
        if _is_torch(data):
            if data.is_cuda:
                torch.cuda.current_stream(data.device).synchronize()
            keep, p = data, data.data_ptr()
        else:
            keep = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
            p = keep.ctypes.data
        if device_out:
            o = torch.empty((max(n_points, 1), 4), dtype=torch.float32, device=f"cuda:{self.device}")
            torch.cuda.synchronize()
            po = o.data_ptr()
        else:
            o = np.empty((max(n_points, 1), 4), np.float32)
            po = o.ctypes.data
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_cloud_from_pointcloud2(self._h, p, n_points, point_step, off_x, off_y, off_z,
                                                     int(is_bigendian), int(not is_dense), po, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_cloud_from_pointcloud2", self._h)
        return o[:m.value]

    def cloud_to_pointxyz(self, xyz1) -> np.ndarray:
        """x,y,z,1 -> the data block (uint8, 16 bytes per point) of a PointCloud2 / pcl::PointCloud<PointXYZ>."""
        p, _k, n = _as_f32(xyz1, 4)
        o = np.empty(16 * max(n, 1), np.uint8)
        rc = _lib.lib().lsgpu_cloud_to_pointxyz(self._h, p, n, o.ctypes.data)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_cloud_to_pointxyz", self._h)
        return o[:16 * n]

    # ---- clouds kept in HBM between calls; sub-map assembly on the device (laser_track.cpp:474-486)
    def cloud_upload(self, slot: int, xyz1, normals=None):
        """normals: the (N, 3) normals the cloud carries (lsgpu_cloud_upload_normals); None: the slot carries none."""
        p, _k, n = _as_f32(xyz1, 4)
        if normals is not None:
            pn, _kn = self._carried(normals, n, "normals")
            rc = _lib.lib().lsgpu_cloud_upload_normals(self._h, slot, p, pn, n)
            if rc != _lib.OK:
                _raise(rc, "lsgpu_cloud_upload_normals", self._h)
            return
        rc = _lib.lib().lsgpu_cloud_upload(self._h, slot, p, n)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_cloud_upload", self._h)

    def cloud_ingest(self, slot: int, cloud, filters, seed: int = -1, normals_knn: int = 0, orient: int = 0,
                     sensor=(0.0, 0.0, 0.0), download: bool = True):
        """lsgpu_cloud_ingest: the raw scan through `filters` (ctypes array of _lib.PointFilter, as apply_point_filters takes
        it) and, with normals_knn > 0, SurfaceNormalDataPointsFilter (+ the orientation pair) on this handle, into `slot`.
        -> (points, normals | None) of the kept cloud, numpy for a host cloud and torch for a device one; download=False:
        nothing comes back, (None, None) -- the cloud is in the slot (cloud_download)."""
        p, _k, n = _as_f32(cloud, 4)
        sv = np.ascontiguousarray(sensor, np.float32).reshape(3)
        o = on = None
        po = pn = None
        if download:
            o, po = self._filter_out(cloud, n)
            if normals_knn:
                if _is_torch(o):
                    on = torch.empty((max(n, 1), 3), dtype=torch.float32, device=o.device)
                    torch.cuda.synchronize()
                    pn = on.data_ptr()
                else:
                    on = np.empty((max(n, 1), 3), np.float32)
                    pn = on.ctypes.data
        m = C.c_int64(0)
        rc = _lib.lib().lsgpu_cloud_ingest(self._h, slot, filters, len(filters), p, n, seed, int(normals_knn), int(orient),
                                           _fp(sv), po, pn, C.byref(m))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_cloud_ingest", self._h)
        if not download:
            return None, None
        return o[:m.value], (on[:m.value] if on is not None else None)

    def cloud_download(self, slot: int):
        """lsgpu_cloud_download: -> (points (N, 4), normals (N, 3) | None) of what the slot holds, as numpy arrays."""
        n = self.cloud_size(slot)
        has = n >= 0 and self.cloud_has_normals(slot)
        o = np.empty((max(n, 1), 4), np.float32)
        on = np.empty((max(n, 1), 3), np.float32) if has else None
        rc = _lib.lib().lsgpu_cloud_download(self._h, slot, o.ctypes.data, on.ctypes.data if has else None, max(n, 0))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_cloud_download", self._h)
        return o[:n], (on[:n] if has else None)

    def cloud_has_normals(self, slot: int) -> bool:
        has = C.c_int(0)
        _lib.lib().lsgpu_cloud_has_normals(self._h, slot, C.byref(has))
        return bool(has.value)

    def cloud_release(self, slot: int):
        _lib.lib().lsgpu_cloud_release(self._h, slot)

    def cloud_size(self, slot: int) -> int:
        n = C.c_int64(-1)
        _lib.lib().lsgpu_cloud_size(self._h, slot, C.byref(n))
        return n.value

    def compute_clouds(self, reading_slot: int, ref_slots, ref_T, T_init, reading_prob: float = 0.5,
                       ssn_knn: int = 10, ssn_ratio: float = 0.5, seed: int = -1, sn_knn: int = 0):
        """ICP::compute with reading = cloud `reading_slot` and reference = concat(T_i * cloud ref_slots[i])."""
        k = len(ref_slots)
        slots = (C.c_int * max(k, 1))(*ref_slots)
        Ts = None
        if ref_T is not None:
            Ts = np.concatenate([_t16(T) for T in ref_T]) if k else np.zeros(0, np.float32)
        ch = _lib.ChainCfg(reading_prob, ssn_knn, ssn_ratio, int(sn_knn), seed)
        ti = _t16(T_init)
        to = np.empty(16, np.float32)
        st = IcpStats()
        rc = _lib.lib().lsgpu_icp_compute_clouds(self._h, reading_slot, slots, _fp(Ts) if Ts is not None else None,
                                                 k, _fp(ti), C.byref(ch), _fp(to), C.byref(st))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_compute_clouds", self._h)
        return to.reshape(4, 4).T.copy(), st

    def compute_clouds_upload(self, reading_slot: int, reading_xyz1, ref_slots, ref_T, T_init, reading_prob: float = 0.5,
                              ssn_knn: int = 10, ssn_ratio: float = 0.5, seed: int = -1, sn_knn: int = 0, reading_normals=None):
        """upload_cloud(reading_slot, reading) + compute_clouds(reading_slot, ...) in one call: the host reading crosses
        PCIe while the sub-map is assembled and filtered (the call shape of LaserTrack::localScanToSubMap).
        reading_normals: the scan is stored with its normals (lsgpu_icp_compute_clouds_upload_normals: upload, then compute)."""
        rd = np.ascontiguousarray(reading_xyz1, np.float32)
        k = len(ref_slots)
        slots = (C.c_int * max(k, 1))(*ref_slots)
        Ts = None
        if ref_T is not None:
            Ts = np.concatenate([_t16(T) for T in ref_T]) if k else np.zeros(0, np.float32)
        ch = _lib.ChainCfg(reading_prob, ssn_knn, ssn_ratio, int(sn_knn), seed)
        ti = _t16(T_init)
        to = np.empty(16, np.float32)
        st = IcpStats()
        if reading_normals is not None:
            pn, _kn = self._carried(np.ascontiguousarray(reading_normals, np.float32), rd.shape[0], "reading_normals")
            rc = _lib.lib().lsgpu_icp_compute_clouds_upload_normals(self._h, reading_slot, rd.ctypes.data if rd.size else None, pn,
                                                                    rd.shape[0], slots, _fp(Ts) if Ts is not None else None, k,
                                                                    _fp(ti), C.byref(ch), _fp(to), C.byref(st))
            if rc != _lib.OK:
                _raise(rc, "lsgpu_icp_compute_clouds_upload_normals", self._h)
            return to.reshape(4, 4).T.copy(), st
        rc = _lib.lib().lsgpu_icp_compute_clouds_upload(self._h, reading_slot, _fp(rd), rd.shape[0], slots,
                                                        _fp(Ts) if Ts is not None else None, k, _fp(ti), C.byref(ch),
                                                        _fp(to), C.byref(st))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_icp_compute_clouds_upload", self._h)
        return to.reshape(4, 4).T.copy(), st

    def trace(self, cap: int = 64):
        buf = (IterTrace * cap)()
        n = _lib.lib().lsgpu_icp_get_trace(self._h, buf, cap)
        out = []
        for i in range(n):
            t = buf[i]
            out.append(dict(T_iter=np.array(t.T_iter[:], np.float32), limit=t.limit,
                            n_used=t.n_used, A=np.array(t.A[:]).reshape(6, 6),
                            b=np.array(t.b[:]), x=np.array(t.x[:]),
                            knn_main_us=t.knn_main_us, knn_fallback_us=t.knn_fallback_us,
                            stragglers=t.stragglers, searching=t.reserved))
        return out

    # ---- kernel-level entry points (reference-mean frame)
    def knn(self, query_xyz1, T=None):
        p, _k, n = _as_f32(query_xyz1, 4)
        ids = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        tp = _fp(_t16(T)) if T is not None else None
        rc = _lib.lib().lsgpu_knn(self._h, p, n, tp, ids.ctypes.data if n else None,
                                  d2.ctypes.data if n else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_knn", self._h)
        return ids, d2

    def knn_k(self, query_xyz1, k: int, T=None):
        """KDTreeMatcher::findClosests with knn = k: (ids, d2), each of shape (n, k) -- row i holds query i's k nearest
        reference points (indices as given to set_reference) in ascending squared distance."""
        p, _k, n = _as_f32(query_xyz1, 4)
        ids = np.empty((n, k), np.int32)
        d2 = np.empty((n, k), np.float32)
        tp = _fp(_t16(T)) if T is not None else None
        rc = _lib.lib().lsgpu_knn_k(self._h, p, n, tp, int(k), ids.ctypes.data if n else None,
                                    d2.ctypes.data if n else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_knn_k", self._h)
        return ids, d2

    def trim_limit(self, d2, ratio: float) -> float:
        a = np.ascontiguousarray(d2, np.float32)
        lim = C.c_float()
        rc = _lib.lib().lsgpu_trim_limit(self._h, a.ctypes.data if a.size else None, a.size,
                                         ratio, C.byref(lim))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_trim_limit", self._h)
        return lim.value

    def normal_eq(self, query_xyz1, T, ids, d2, limit: float):
        """-> (A 6x6, b 6, n_used, sum r^2), double."""
        p, _k, n = _as_f32(query_xyz1, 4)
        ids = np.ascontiguousarray(ids, np.int32)
        d2 = np.ascontiguousarray(d2, np.float32)
        out = np.zeros(29)
        tp = _fp(_t16(T)) if T is not None else None
        rc = _lib.lib().lsgpu_normal_eq(self._h, p, n, tp, ids.ctypes.data, d2.ctypes.data, limit,
                                        out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_normal_eq", self._h)
        A = np.zeros((6, 6))
        k = 0
        for a in range(6):
            for c in range(a, 6):
                A[a, c] = A[c, a] = out[k]
                k += 1
        return A, out[21:27].copy(), int(out[27]), float(out[28])

    def point_to_point(self, query_xyz1, T, ids, d2, limit: float) -> np.ndarray:
        """lsgpu_point_to_point: the 29 point-to-point sums (sum p, sum q, sum q p^T row major, 12 zeros, count,
        sum |p - q|^2) of the pairs with d2 <= limit, double."""
        p, _k, n = _as_f32(query_xyz1, 4)
        ids = np.ascontiguousarray(ids, np.int32)
        d2 = np.ascontiguousarray(d2, np.float32)
        out = np.zeros(29)
        tp = _fp(_t16(T)) if T is not None else None
        rc = _lib.lib().lsgpu_point_to_point(self._h, p, n, tp, ids.ctypes.data, d2.ctypes.data, limit,
                                             out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != _lib.OK:
            _raise(rc, "lsgpu_point_to_point", self._h)
        return out

    def transform_points(self, T, xyz1):
        p, _k, n = _as_f32(xyz1, 4)
        out = np.empty((n, 4), np.float32)
        rc = _lib.lib().lsgpu_transform_points(self._h, _fp(_t16(T)), p, n,
                                               out.ctypes.data if n else None)
        if rc != _lib.OK:
            _raise(rc, "lsgpu_transform_points", self._h)
        return out


def _rotate_descriptors(self, T, desc3):
    """RigidTransformation::compute on a 3-row descriptor (normals / observationDirections): R * d on the device."""
    p, _k, n = _as_f32(desc3, 3)
    out = np.empty((n, 3), np.float32)
    rc = _lib.lib().lsgpu_rotate_descriptors(self._h, _fp(_t16(T)), p, n, out.ctypes.data if n else None)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_rotate_descriptors", self._h)
    return out


IcpHandle.rotate_descriptors = _rotate_descriptors


def align_batch(handles, references, normals, readings, T_inits):
    """BASELINE config 3: many independent pairs on one GPU (``lsgpu_icp_align_batch``).

    ``handles``: IcpHandle pool on one device (pair i -> handles[i % len]); every cloud may be a host
    array or a CUDA tensor.  -> (T [B,4,4] float32, [IcpStats], rc int array); non-converged pairs keep
    T_init and have rc == 1, any other failure raises."""
    B = len(readings)
    if not (len(references) == len(normals) == len(T_inits) == B):
        raise ValueError("one reference, normals, reading and T_init per pair")
    keep, rp, npn, qp = [], (C.c_void_p * B)(), (C.c_void_p * B)(), (C.c_void_p * B)()
    nr, nq = (C.c_int64 * B)(), (C.c_int64 * B)()
    for i in range(B):
        p, k1, n = _as_f32(references[i], 4)
        q, k2, m = _as_f32(normals[i], 3) if normals[i] is not None else (None, None, n)   # (None: point-to-point handles)
        r, k3, l = _as_f32(readings[i], 4)
        if m != n:
            raise ValueError("normals must have one row per reference point")
        keep += [k1, k2, k3]
        rp[i], npn[i], qp[i], nr[i], nq[i] = p, q, r, n, l
    ti = np.concatenate([_t16(T) for T in T_inits]) if B else np.zeros(0, np.float32)
    to = np.empty(16 * B, np.float32)
    st = (IcpStats * max(B, 1))()
    rc = (C.c_int * max(B, 1))()
    hs = (C.c_void_p * len(handles))(*[h._h for h in handles])
    code = _lib.lib().lsgpu_icp_align_batch(hs, len(handles), B, rp, npn, nr, qp, nq, _fp(ti), _fp(to), st, rc)
    if code not in (_lib.OK, _lib.NO_CONVERGENCE):
        bad = next((i for i in range(B) if rc[i] not in (_lib.OK, _lib.NO_CONVERGENCE)), None)
        _raise(code, "lsgpu_icp_align_batch" + (f" (pair {bad})" if bad is not None else ""),
               handles[bad % len(handles)]._h if bad is not None else None)
    T = to.reshape(B, 4, 4).transpose(0, 2, 1).copy()
    return T, [st[i] for i in range(B)], np.array(rc[:B], np.int32)


def comm_unique_id() -> bytes:
    """RCCL unique id (call on rank 0, ship to the other ranks)."""
    buf = C.create_string_buffer(128)
    rc = _lib.lib().lsgpu_comm_get_unique_id(buf)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_comm_get_unique_id")
    return buf.raw


# ---------------------------------------------------------------------------------------------
# host-side modules (CPU in the reference too)

def random_sampling(n: int, prob: float, seed: int = -1) -> np.ndarray:
    """RandomSamplingDataPointsFilter (icp_default.yaml:1-3) -> kept indices."""
    keep = np.empty(max(n, 1), np.int64)
    m = _lib.lib().lsgpu_filter_random_sampling(n, prob, seed,
                                                keep.ctypes.data_as(C.POINTER(C.c_int64)))
    return keep[:m].copy()


def sampling_surface_normal(xyz1, knn: int = 10, ratio: float = 0.5, seed: int = -1):
    """SamplingSurfaceNormalDataPointsFilter (icp_default.yaml:5-7) -> (xyz1', normals)."""
    a = np.ascontiguousarray(xyz1, np.float32)
    n = a.shape[0]
    o = np.empty((max(n, 1), 4), np.float32)
    nr = np.empty((max(n, 1), 3), np.float32)
    m = _lib.lib().lsgpu_filter_sampling_surface_normal(a.ctypes.data if n else None, n, knn, ratio,
                                                        seed, o.ctypes.data, nr.ctypes.data)
    return o[:m].copy(), nr[:m].copy()


def surface_normal(xyz1, knn: int = 5, with_neighbours: bool = False, with_densities: bool = False):
    """SurfaceNormalDataPointsFilter on the host (lsgpu_filter_surface_normal; the device filter's checker, bit for bit)
    -> normals (n, 3), or (normals, ids (n, knn), d2 (n, knn)) with `with_neighbours`; with_densities (keepDensities 1)
    appends the densities (n,)."""
    a = np.ascontiguousarray(xyz1, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"expected (N,4) array, got {a.shape}")
    n = a.shape[0]
    knn = int(knn)
    if not 3 <= knn <= 32:
        raise LsgpuError(_lib.BAD_ARG, "lsgpu_filter_surface_normal", "knn must be in [3, 32]")
    nr = np.empty((max(n, 1), 3), np.float32)
    ids = np.empty((max(n, 1), max(knn, 1)), np.int32) if with_neighbours else None
    d2 = np.empty((max(n, 1), max(knn, 1)), np.float32) if with_neighbours else None
    dn = np.empty((max(n, 1),), np.float32) if with_densities else None
    rc = _lib.lib().lsgpu_filter_surface_normal_densities(a.ctypes.data if n else None, n, int(knn), nr.ctypes.data,
                                                          ids.ctypes.data if with_neighbours else None,
                                                          d2.ctypes.data if with_neighbours else None,
                                                          dn.ctypes.data if with_densities else None)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_filter_surface_normal")
    out = (nr[:n], ids[:n], d2[:n]) if with_neighbours else (nr[:n],)
    if with_densities:
        out += (dn[:n],)
    return out if len(out) > 1 else out[0]


def max_density(xyz1, knn: int = 10, max_density: float = 10.0, seed: int = -1):
    """SurfaceNormalDataPointsFilter keepDensities 1 + MaxDensityDataPointsFilter on the host (lsgpu_filter_max_density; the
    device pass's checker, bit for bit) -> (xyz1', normals, n_dense, densities of the input points).  Raises ConvergenceError
    if nothing is kept (the draws are consumed all the same)."""
    a = np.ascontiguousarray(xyz1, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"expected (N,4) array, got {a.shape}")
    n = a.shape[0]
    o = np.empty((max(n, 1), 4), np.float32)
    nr = np.empty((max(n, 1), 3), np.float32)
    dn = np.empty((max(n, 1),), np.float32)
    m, nd = C.c_int64(0), C.c_int64(0)
    rc = _lib.lib().lsgpu_filter_max_density(a.ctypes.data if n else None, n, int(knn), float(max_density), seed, o.ctypes.data,
                                             nr.ctypes.data, dn.ctypes.data, C.byref(m), C.byref(nd))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_filter_max_density")
    return o[:m.value].copy(), nr[:m.value].copy(), nd.value, dn[:n]


def shadow(xyz1, normals, eps: float = 0.1):
    """ShadowDataPointsFilter on the host (lsgpu_filter_shadow; the device pass's checker, bit for bit) -> (xyz1', normals').
    Raises ConvergenceError if nothing is kept."""
    a = np.ascontiguousarray(xyz1, np.float32)
    b = np.ascontiguousarray(normals, np.float32)
    if a.ndim != 2 or a.shape[1] != 4 or b.ndim != 2 or b.shape[1] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError(f"expected (N,4) points and (N,3) normals, got {a.shape} and {b.shape}")
    n = a.shape[0]
    o = np.empty((max(n, 1), 4), np.float32)
    nr = np.empty((max(n, 1), 3), np.float32)
    k = C.c_int64(0)
    rc = _lib.lib().lsgpu_filter_shadow(a.ctypes.data if n else None, b.ctypes.data if n else None, n, float(eps), o.ctypes.data,
                                        nr.ctypes.data, C.byref(k))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_filter_shadow")
    return o[:k.value].copy(), nr[:k.value].copy()


def _c_int(v) -> int:
    """An integer parameter on its way into a C int: a value that is no integer is refused here, one out of an int's range is
    clamped to a value the library refuses all the same."""
    if int(v) != v:
        raise ValueError(f"expected an integer, got {v!r}")
    return min(max(int(v), -(2 ** 31)), 2 ** 31 - 1)


def cov_sampling(xyz1, normals, nb_sample: int = 5000, torque_norm: int = 1, sums=None, return_sums: bool = False):
    """CovarianceSamplingDataPointsFilter on the host (lsgpu_filter_cov_sampling) -> (xyz1', normals', ids) in pick order, with
    return_sums also the 32 sums used.  sums: None -- the twin adds its own, sequentially -- or the 32 doubles of
    IcpHandle.filter_cov_sampling(return_sums=True): fed those, the twin is the device path's checker, bit for bit."""
    a = np.ascontiguousarray(xyz1, np.float32)
    b = np.ascontiguousarray(normals, np.float32)
    if a.ndim != 2 or a.shape[1] != 4 or b.ndim != 2 or b.shape[1] != 3 or a.shape[0] != b.shape[0]:
        raise ValueError(f"expected (N,4) points and (N,3) normals, got {a.shape} and {b.shape}")
    n = a.shape[0]
    nb = _c_int(nb_sample)
    room = max(min(nb, n), 1)
    o = np.empty((room, 4), np.float32)
    nr = np.empty((room, 3), np.float32)
    ids = np.empty((room,), np.int32)
    s_in = None
    if sums is not None:
        s_in = np.ascontiguousarray(sums, np.float64)
        if s_in.shape != (32,):
            raise ValueError(f"expected 32 sums, got {s_in.shape}")
    s_out = np.zeros(32, np.float64)
    k = C.c_int64(0)
    rc = _lib.lib().lsgpu_filter_cov_sampling(a.ctypes.data if n else None, b.ctypes.data if n else None, n, nb, _c_int(torque_norm),
                                              s_in.ctypes.data if s_in is not None else None, o.ctypes.data, nr.ctypes.data,
                                              ids.ctypes.data, C.byref(k), s_out.ctypes.data)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_filter_cov_sampling")
    out = (o[:k.value].copy(), nr[:k.value].copy(), ids[:k.value].copy())
    return out + (s_out,) if return_sums else out


def cov_sampling_eigen(C21):
    """lsgpu_cov_sampling_eigen: the cyclic Jacobi of CovarianceSamplingDataPointsFilter on the upper triangle (21 doubles, row
    major) of a symmetric 6x6 matrix -> (X, values): X (6, 6) float32 with the k-th eigenvector in column k, values ascending."""
    c = np.ascontiguousarray(C21, np.float64)
    if c.shape != (21,):
        raise ValueError(f"expected 21 values, got {c.shape}")
    X = np.empty((6, 6), np.float32)
    w = np.empty(6, np.float64)
    rc = _lib.lib().lsgpu_cov_sampling_eigen(c.ctypes.data, X.ctypes.data, w.ctypes.data)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_cov_sampling_eigen")
    return X, w


def cov_sampling_cfg(c) -> "_lib.CovSamplingCfg":
    """((reading_nb_sample, reading_torque_norm) or None, (reference_nb_sample, reference_torque_norm) or None) / a dict of
    lsgpu_cov_sampling_config's fields / an _lib.CovSamplingCfg -> _lib.CovSamplingCfg (the values are checked by the library)."""
    if isinstance(c, _lib.CovSamplingCfg):
        return c
    out = _lib.CovSamplingCfg()
    _lib.lib().lsgpu_cov_sampling_config_default(C.byref(out))
    if isinstance(c, dict):
        for k, v in c.items():
            if k not in ("reading_nb_sample", "reference_nb_sample", "reading_torque_norm", "reference_torque_norm"):
                raise ValueError(f"lsgpu_cov_sampling_config has no field {k}")
            setattr(out, k, _c_int(v))
        return out
    rd, ref = c
    if rd is not None:
        out.reading_nb_sample, out.reading_torque_norm = _c_int(rd[0]), _c_int(rd[1])
    if ref is not None:
        out.reference_nb_sample, out.reference_torque_norm = _c_int(ref[0]), _c_int(ref[1])
    return out


def _cov_sampling_pairs(cc):
    """_lib.CovSamplingCfg -> ((nbSample, torqueNorm) or None of the reading, the same of the reference), None: no module."""
    rd = (int(cc.reading_nb_sample), int(cc.reading_torque_norm)) if cc.reading_nb_sample > 0 else None
    ref = (int(cc.reference_nb_sample), int(cc.reference_torque_norm)) if cc.reference_nb_sample > 0 else None
    return (rd, ref) if rd or ref else None


def shadow_cfg(s) -> "_lib.ShadowCfg":
    """(reading_eps, reference_eps) / a dict with those keys / an _lib.ShadowCfg -> _lib.ShadowCfg (None or a negative eps: -1)."""
    if isinstance(s, _lib.ShadowCfg):
        return s
    if isinstance(s, dict):
        s = (s.get("reading_eps"), s.get("reference_eps"))
    rd, ref = s
    c = _lib.ShadowCfg()
    _lib.lib().lsgpu_shadow_config_default(C.byref(c))
    if rd is not None and not rd < 0:
        c.reading_eps = float(rd)
    if ref is not None and not ref < 0:
        c.reference_eps = float(ref)
    return c


def voxel_grid_points(xyz1, vsize=(1.0, 1.0, 1.0), use_centroid: bool = True) -> np.ndarray:
    """VoxelGridDataPointsFilter of the input filter chain on the host (lsgpu_filter_voxel_grid_points; bit for bit what
    IcpHandle.apply_point_filters gives with this one module) -> one point per occupied voxel, in first-point order."""
    a = np.ascontiguousarray(xyz1, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"expected (N,4) array, got {a.shape}")
    n = a.shape[0]
    v = (C.c_float * 3)(*[float(x) for x in vsize])
    o = np.empty((max(n, 1), 4), np.float32)
    m = _lib.lib().lsgpu_filter_voxel_grid_points(a.ctypes.data if n else None, n, v, int(use_centroid), o.ctypes.data)
    if m < 0:
        _raise(int(-m), "lsgpu_filter_voxel_grid_points")
    return o[:m].copy()


def octree_grid_points(xyz1, max_size_by_node: float = 0.0, max_point_by_node: int = 1, sampling_method: int = 0,
                       seed: int = -1) -> np.ndarray:
    """OctreeGridDataPointsFilter of the input filter chain on the host (lsgpu_filter_octree_grid_points; bit for bit what
    IcpHandle.apply_point_filters gives with this one module) -> one point per non-empty leaf, in depth-first leaf order.
    sampling_method: 0 FirstPts, 1 RandomPts (one draw of the library's stream per leaf; seed >= 0 reseeds it first),
    2 Centroid, 3 Medoid."""
    a = np.ascontiguousarray(xyz1, np.float32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"expected (N,4) array, got {a.shape}")
    if int(max_point_by_node) != max_point_by_node:
        raise ValueError("max_point_by_node must be an integer")
    n = a.shape[0]
    o = np.empty((max(n, 1), 4), np.float32)
    m = _lib.lib().lsgpu_filter_octree_grid_points(a.ctypes.data if n else None, n, float(max_size_by_node),
                                                   min(max(int(max_point_by_node), -1), 2 ** 31 - 1),   # (a C int; refused all the same)
                                                   int(sampling_method), int(seed), o.ctypes.data)
    if m < 0:
        _raise(int(-m), "lsgpu_filter_octree_grid_points")
    return o[:m].copy()


def point_to_point_solve(sums) -> np.ndarray:
    """lsgpu_point_to_point_solve: the point-to-point step dT (4x4 float32) from the 29 sums of
    IcpHandle.point_to_point -- host only, the same function the device loop runs.  Raises ConvergenceError for
    count 0."""
    s = np.ascontiguousarray(sums, np.float64)
    if s.shape != (29,):
        raise ValueError("expected 29 sums")
    out = np.empty(16, np.float32)
    rc = _lib.lib().lsgpu_point_to_point_solve(s.ctypes.data_as(C.POINTER(C.c_double)), _fp(out))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_point_to_point_solve")
    return out.reshape(4, 4).T.copy()


def point_to_plane_solve(sums) -> np.ndarray:
    """lsgpu_point_to_plane_solve: the point-to-plane step dT (4x4 float32) from the first 27 sums of lsgpu_normal_eq --
    host only, the same function the device loop runs.  Raises ConvergenceError if A is not positive definite."""
    s = np.ascontiguousarray(sums, np.float64).ravel()
    if s.size < 27:
        raise ValueError("expected at least 27 sums")
    out = np.empty(16, np.float32)
    rc = _lib.lib().lsgpu_point_to_plane_solve(s.ctypes.data_as(C.POINTER(C.c_double)), _fp(out))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_point_to_plane_solve")
    return out.reshape(4, 4).T.copy()


def point_to_plane_solve_dof(sums, dof: int) -> np.ndarray:
    """lsgpu_point_to_plane_solve_dof: the step dT (4x4 float32) of a handle's mode from the first 27 sums of lsgpu_normal_eq --
    dof _lib.MOTION_DOF_6 (the free step), _lib.MOTION_DOF_4 (force4DOF) or _lib.MOTION_DOF_3 (force2D; b formed with the planar
    residual).  Host only, the function the device loop runs.  Raises ConvergenceError if the system is not positive definite."""
    s = np.ascontiguousarray(sums, np.float64).ravel()
    if s.size < 27:
        raise ValueError("expected at least 27 sums")
    out = np.empty(16, np.float32)
    rc = _lib.lib().lsgpu_point_to_plane_solve_dof(s.ctypes.data_as(C.POINTER(C.c_double)), int(dof), _fp(out))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_point_to_plane_solve_dof")
    return out.reshape(4, 4).T.copy()


def bound_first_violation(T_iters, max_rot: float, max_trans: float) -> int:
    """lsgpu_bound_first_violation: BoundTransformationChecker over a sequence of 4x4 transforms (entry 0: the one the checker
    was initialised with) -> the first index >= 1 out of bounds, -1 if there is none.  Host only."""
    Ts = [np.asarray(T, np.float32).reshape(4, 4).T.ravel() for T in T_iters]          # column major
    a = np.ascontiguousarray(np.concatenate(Ts) if Ts else np.zeros(0), np.float32)
    return int(_lib.lib().lsgpu_bound_first_violation(a.ctypes.data if len(Ts) else None, len(Ts), float(max_rot), float(max_trans)))


def point_to_plane_cov_solve(sums, sensor_std_dev: float = 0.01) -> np.ndarray:
    """lsgpu_point_to_plane_cov_solve: cov = sensorStdDev^2 H^-1 M H^-1 (6x6 float64) from the 44 sums of
    IcpHandle.point_to_plane_cov -- host only, the function the library calls after the loop.  Raises ConvergenceError for
    a pair count of 0, a non-finite sum or a singular H."""
    s = np.ascontiguousarray(sums, np.float64)
    if s.shape != (44,):
        raise ValueError("expected 44 sums")
    out = np.empty(36, np.float64)
    rc = _lib.lib().lsgpu_point_to_plane_cov_solve(s.ctypes.data_as(C.POINTER(C.c_double)), float(sensor_std_dev),
                                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_point_to_plane_cov_solve")
    return out.reshape(6, 6)


@dataclass
class RobustConfig:
    """RobustOutlierFilter's parameters, with the module's defaults."""
    robust_fct: str = "cauchy"
    tuning: float = 1.0
    scale_estimator: str = "mad"
    nb_iteration_for_scale: int = 0
    distance_type: str = "point2point"
    approximation: float = math.inf


def robust_cfg(r) -> "_lib.RobustCfg":
    """RobustConfig / dict of its fields / _lib.RobustCfg -> _lib.RobustCfg.  Unknown names raise (bad config)."""
    if isinstance(r, _lib.RobustCfg):
        return r
    if isinstance(r, dict):
        r = RobustConfig(**r)
    for table, v, what in ((_lib.ROBUST_FCT, r.robust_fct, "robustFct"), (_lib.ROBUST_SCALE, r.scale_estimator, "scaleEstimator"),
                           (_lib.ROBUST_DIST, r.distance_type, "distanceType")):
        if v not in table:
            raise LsgpuError(_lib.BAD_CONFIG, "RobustOutlierFilter", f"RobustOutlierFilter: unknown {what} {v}")
    return _lib.RobustCfg(_lib.ROBUST_FCT[r.robust_fct], float(r.tuning), _lib.ROBUST_SCALE[r.scale_estimator],
                          int(r.nb_iteration_for_scale), _lib.ROBUST_DIST[r.distance_type], float(r.approximation))


@dataclass
class NormalsConfig:
    """lsgpu_normals_config: SurfaceNormalOutlierFilter (max_angle < 0: none), SurfaceNormalDataPointsFilter on the reading
    (reading_sn_knn, 0: none), the orientation pairs (0 off, 1 towardCenter, 2 away) and their sensor positions."""
    max_angle: float = -1.0
    reading_sn_knn: int = 0
    reading_orient: int = 0
    reference_orient: int = 0
    reading_sensor: tuple = (0.0, 0.0, 0.0)
    reference_sensor: tuple = (0.0, 0.0, 0.0)
    reading_normals_given: int = 0


def normals_cfg(n) -> "_lib.NormalsCfg":
    if isinstance(n, _lib.NormalsCfg):
        return n
    if isinstance(n, dict):
        n = NormalsConfig(**n)
    c = _lib.NormalsCfg()
    c.max_angle = float(n.max_angle)
    c.reading_sn_knn, c.reading_orient, c.reference_orient = int(n.reading_sn_knn), int(n.reading_orient), int(n.reference_orient)
    for i in range(3):
        c.reading_sensor[i] = float(n.reading_sensor[i])
        c.reference_sensor[i] = float(n.reference_sensor[i])
    c.reading_normals_given = int(n.reading_normals_given)
    return c


def orient_normals(xyz1, normals, sensor, toward_center: bool = True) -> np.ndarray:
    """lsgpu_orient_normals: the orientation step on the host -- the device's, bit for bit.  Returns the oriented copy."""
    p = np.ascontiguousarray(xyz1, np.float32)
    out = np.ascontiguousarray(normals, np.float32).copy()
    sv = np.asarray(sensor, np.float32)
    rc = _lib.lib().lsgpu_orient_normals(p.ctypes.data if p.size else None, len(p), _fp(sv), 1 if toward_center else 2,
                                         out.ctypes.data if out.size else None)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_orient_normals")
    return out


def normal_angle_weights(T, reading_normals, reference_normals, ids, max_angle: float) -> np.ndarray:
    """lsgpu_normal_angle_weights: SurfaceNormalOutlierFilter's 0 / 1 weights (ids: n or n x k) -- the device loop's."""
    rn = np.ascontiguousarray(reading_normals, np.float32)
    fn = np.ascontiguousarray(reference_normals, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    k = 1 if idv.ndim == 1 else idv.shape[1]
    w = np.empty(idv.shape, np.float32)
    rc = _lib.lib().lsgpu_normal_angle_weights(_fp(_t16(T)), rn.ctypes.data if rn.size else None, len(rn), fn.ctypes.data if fn.size else None,
                                               idv.ctypes.data if idv.size else None, k, float(max_angle),
                                               w.ctypes.data if w.size else None)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_normal_angle_weights")
    return w


def robust_scale(d2):
    """lsgpu_robust_scale: (median, MAD scale) of the finite entries of d2, float32 -- the device loop's, bit for bit."""
    a = np.ascontiguousarray(d2, np.float32).ravel()
    med, sc = C.c_float(), C.c_float()
    rc = _lib.lib().lsgpu_robust_scale(a.ctypes.data if a.size else None, a.size, C.byref(med), C.byref(sc))
    if rc != _lib.OK:
        _raise(rc, "lsgpu_robust_scale")
    return np.float32(med.value), np.float32(sc.value)


def robust_weights(robust, scale, e) -> np.ndarray:
    """lsgpu_robust_weights: the weights of e (d2, or r r for point2plane) -- the device loop's, bit for bit."""
    rb = robust_cfg(robust)
    a = np.ascontiguousarray(e, np.float32).ravel()
    w = np.empty(a.size, np.float32)
    rc = _lib.lib().lsgpu_robust_weights(C.byref(rb), float(scale), a.ctypes.data if a.size else None, a.size,
                                         w.ctypes.data if a.size else None)
    if rc != _lib.OK:
        _raise(rc, "lsgpu_robust_weights")
    return w


def check_rigid(T) -> bool:
    return bool(_lib.lib().lsgpu_check_rigid(_fp(_t16(T))))


def rotation_distance(Ta, Tb) -> float:
    """DifferentialTransformationChecker's rotation metric between two transforms (Eigen angularDistance, float)."""
    return float(_lib.lib().lsgpu_rotation_distance(_fp(_t16(Ta)), _fp(_t16(Tb))))


def correct_rigid(T) -> np.ndarray:
    out = np.empty(16, np.float32)
    _lib.lib().lsgpu_correct_rigid(_fp(_t16(T)), _fp(out))
    return out.reshape(4, 4).T.copy()


# ---------------------------------------------------------------------------------------------

_MINIMIZERS = {"PointToPlaneErrorMinimizer": _lib.MINIMIZER_POINT_TO_PLANE,
               "PointToPointErrorMinimizer": _lib.MINIMIZER_POINT_TO_POINT}


@dataclass
class ChainConfig:
    """The module chain of laser_slam/configurations/icp_default.yaml, as parameters."""
    reading_sampling_prob: float = 0.5      # yaml:3   (module default 0.75)
    surface_normal_knn: int = 10            # yaml:7   (module default 7); 0: no reference filter (point-to-point only)
    surface_normal_ratio: float = 0.5       # module default
    reference_normal_knn: int = 0           # SurfaceNormalDataPointsFilter knn (module default 5) as the reference filter; 0: absent
    trim_ratio: float = 0.75                # yaml:16  (module default 0.85)
    max_iterations: int = 40                # yaml:23
    min_diff_rot: float = 0.001             # yaml:25
    min_diff_trans: float = 0.01            # yaml:26  (module default 0.001)
    smooth_length: int = 4                  # yaml:27  (module default 3)
    seed: int = -1                          # >= 0: srand(seed) before the filters
    error_minimizer: str = "PointToPlaneErrorMinimizer"   # yaml:18-19, or "PointToPointErrorMinimizer"
    matcher_knn: int = 1                    # yaml:11  KDTreeMatcher knn (1.._lib.MATCHER_KNN_MAX), epsilon 0
    matcher_max_dist: float = 0.0           # KDTreeMatcher maxDist [m]; 0: absent (inf)
    outlier_max_dist: float = 0.0           # MaxDistOutlierFilter maxDist [m]; 0: no such module
    outlier_min_dist: float = 0.0           # MinDistOutlierFilter minDist [m]; 0: no such module (or minDist 0: keeps all)
    outlier_median_factor: float = 0.0      # MedianDistOutlierFilter factor; 0: no such module
    extra: dict = field(default_factory=dict)   # "robust": RobustOutlierFilter's parameters (see `robust`); "normals": see `normals`; "cuts": see `cuts`

    @property
    def cuts(self) -> Optional["ChainCuts"]:
        """The cut modules of the two filter sections (a ChainCuts); None: none.  Kept in `extra`, like `robust`, so that a
        chain without them compares equal to what it was."""
        return self.extra.get("cuts")

    @cuts.setter
    def cuts(self, value):
        if value is None:
            self.extra.pop("cuts", None)
        else:
            self.extra["cuts"] = value

    @property
    def normals(self) -> Optional["NormalsConfig"]:
        """SurfaceNormalOutlierFilter / reading normals / oriented normals (a NormalsConfig); None: none of these modules.
        Kept in `extra`, like `robust`."""
        return self.extra.get("normals")

    @normals.setter
    def normals(self, value):
        if value is None:
            self.extra.pop("normals", None)
        else:
            self.extra["normals"] = value

    @property
    def covariance(self) -> Optional[float]:
        """PointToPlaneWithCovErrorMinimizer's sensorStdDev; None: the covariance is not asked for.  The step is
        PointToPlaneErrorMinimizer's: `error_minimizer` names that module.  Kept in `extra`, like `robust`."""
        return self.extra.get("covariance")

    @covariance.setter
    def covariance(self, value):
        if value is None:
            self.extra.pop("covariance", None)
        else:
            self.extra["covariance"] = float(value)

    @property
    def max_density(self) -> Optional[float]:
        """MaxDensityDataPointsFilter's maxDensity behind the reference's SurfaceNormalDataPointsFilter with keepDensities 1
        (`reference_normal_knn`); None: no such module.  Kept in `extra`, like `robust`."""
        return self.extra.get("max_density")

    @max_density.setter
    def max_density(self, value):
        if value is None:
            self.extra.pop("max_density", None)
        else:
            self.extra["max_density"] = float(value)

    @property
    def shadow(self):
        """ShadowDataPointsFilter's eps of the two filter sections, (reading_eps or None, reference_eps or None); None: no
        such module.  Kept in `extra`, like `robust`."""
        return self.extra.get("shadow")

    @shadow.setter
    def shadow(self, value):
        if value is None or (value[0] is None and value[1] is None):
            self.extra.pop("shadow", None)
        else:
            self.extra["shadow"] = (None if value[0] is None else float(value[0]), None if value[1] is None else float(value[1]))

    @property
    def cov_sampling(self):
        """CovarianceSamplingDataPointsFilter of the two filter sections, ((nbSample, torqueNorm) or None of the reading, the
        same of the reference); None: no such module.  Kept in `extra`, like `robust`."""
        return self.extra.get("cov_sampling")

    @cov_sampling.setter
    def cov_sampling(self, value):
        if value is None:
            self.extra.pop("cov_sampling", None)
        else:
            self.extra["cov_sampling"] = tuple(None if v is None else (int(v[0]), int(v[1])) for v in value)

    @property
    def motion(self) -> Optional["MotionConfig"]:
        """PointToPlaneErrorMinimizer's force2D / force4DOF and BoundTransformationChecker (a MotionConfig); None: neither.
        Kept in `extra`, like `robust`."""
        return self.extra.get("motion")

    @motion.setter
    def motion(self, value):
        if value is None:
            self.extra.pop("motion", None)
        else:
            self.extra["motion"] = value

    @property
    def robust(self) -> Optional["RobustConfig"]:
        """RobustOutlierFilter's parameters (a RobustConfig); None: no such module.  Kept in `extra`, so that the fields of
        a chain without the module are what they were."""
        return self.extra.get("robust")

    @robust.setter
    def robust(self, value):
        if value is None:
            self.extra.pop("robust", None)
        else:
            self.extra["robust"] = value


@dataclass(frozen=True)
class MotionConfig:
    """lsgpu_motion_config: `dof` _lib.MOTION_DOF_6 (the free step), _lib.MOTION_DOF_3 (PointToPlaneErrorMinimizer force2D) or
    _lib.MOTION_DOF_4 (force4DOF); `bound`: BoundTransformationChecker with its two limits (rad, m), `bound_before_counter`:
    the document lists it in front of CounterTransformationChecker (the counter's last iteration is checked too)."""
    dof: int = 0
    bound: bool = False
    max_rotation_norm: float = 1.0
    max_translation_norm: float = 1.0
    bound_before_counter: bool = False


def motion_cfg(m) -> "_lib.MotionCfg":
    """MotionConfig / dict of its fields / _lib.MotionCfg -> _lib.MotionCfg (the values are checked by the library)."""
    if isinstance(m, _lib.MotionCfg):
        return m
    if isinstance(m, dict):
        m = MotionConfig(**m)
    c = _lib.MotionCfg()
    _lib.lib().lsgpu_motion_config_default(C.byref(c))
    c.dof, c.bound, c.bound_before_counter = int(m.dof), int(m.bound), int(m.bound_before_counter)
    c.max_rotation_norm, c.max_translation_norm = float(m.max_rotation_norm), float(m.max_translation_norm)
    return c


def _motion_config(mc) -> "MotionConfig":
    """_lib.MotionCfg -> MotionConfig"""
    return MotionConfig(int(mc.dof), bool(mc.bound), _f32(mc.max_rotation_norm), _f32(mc.max_translation_norm),
                        bool(mc.bound_before_counter))


@dataclass(frozen=True)
class ChainCuts:
    """lsgpu_chain_cuts: the cut modules of an ICP chain's filter sections, each `(type, dim, flag, (v, ...))` with type one
    of _lib.FILTER_MAX_DIST / _MIN_DIST / _BOUNDING_BOX / _REMOVE_NAN, in the document's order.  `reading_sampling_at`: how
    many of the reading's stand in front of RandomSampling (not read on a chain without it)."""
    reading: tuple = ()
    reference: tuple = ()
    reading_sampling_at: int = 0


def chain_cuts_cfg(c) -> "_lib.ChainCuts":
    """ChainCuts / dict of its fields / _lib.ChainCuts -> _lib.ChainCuts (the counts are checked by the library)."""
    if isinstance(c, _lib.ChainCuts):
        return c
    if isinstance(c, dict):
        c = ChainCuts(tuple(c.get("reading", ())), tuple(c.get("reference", ())), int(c.get("reading_sampling_at", 0)))
    out = _lib.ChainCuts()
    out.n_reading, out.n_reference, out.reading_sampling_at = len(c.reading), len(c.reference), int(c.reading_sampling_at)
    for dst, mods in ((out.reading, c.reading), (out.reference, c.reference)):
        for f, (typ, dim, flag, v) in zip(dst, mods):     # (more than CHAIN_CUT_MAX: the count says so, the library refuses it)
            f.type, f.dim, f.flag = int(typ), int(dim), int(flag)
            for i, x in enumerate(tuple(v)[:6]):
                f.v[i] = float(x)
    return out


def _chain_cuts(cc) -> "ChainCuts":
    """_lib.ChainCuts -> ChainCuts"""
    mods = lambda arr, n: tuple((f.type, f.dim, f.flag, tuple(_f32(x) for x in f.v)) for f in arr[:n])
    return ChainCuts(mods(cc.reading, cc.n_reading), mods(cc.reference, cc.n_reference), cc.reading_sampling_at)


def _yaml_modules(doc):
    """A YAML chain document read with yaml.BaseLoader -> (lsgpu_yaml_module array, count, what keeps its strings alive)."""
    mods = []
    for section, v in doc.items():
        for it in (v if isinstance(v, list) else [v]):
            if isinstance(it, str) and it:                      # `- Name` / `section: Name`
                mods.append((section, it, {}))
            elif isinstance(it, dict):                          # `- Name: {params}` / `Name:` with an indented block
                mods += [(section, name, p if isinstance(p, dict) else {}) for name, p in it.items()]
    arr = (_lib.YamlModule * max(len(mods), 1))()
    keep = []
    for a, (section, name, params) in zip(arr, mods):
        kv = sorted((str(k).encode(), str(v).encode()) for k, v in params.items())   # by key, as the C++ facade's std::map
        ps = (_lib.YamlParam * max(len(kv), 1))(*[_lib.YamlParam(k, v) for k, v in kv])
        keep.append(ps)
        a.section, a.name, a.params, a.n_params = str(section).encode(), str(name).encode(), ps, len(kv)
    return arr, len(mods), keep


def chain_load(doc, carried: int = 0):
    """lsgpu_chain_load on a YAML chain document read with yaml.BaseLoader (every scalar stays text): its modules, section by
    section in the document's order -> (return code, reason of a refusal, _lib.LoadedChain).  The rules are the library's.
    carried != 0: lsgpu_chain_load_carried -- the caller's clouds carry normals (_lib.CARRIED_READING | _lib.CARRIED_REFERENCE)."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.LoadedChain()
    why = C.create_string_buffer(512)
    if carried:
        rc = _lib.lib().lsgpu_chain_load_carried(arr, n, int(carried), C.byref(out), why, len(why))
    else:
        rc = _lib.lib().lsgpu_chain_load(arr, n, C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def chain_load_parts_carried(doc, carried: int):
    """lsgpu_chain_load_parts_carried: what chain_load_cuts, _shadow, _motion and _cov_sampling give, for a caller whose clouds
    carry normals -> (return code, reason of a refusal, _lib.ChainCuts, _lib.ShadowCfg, _lib.MotionCfg, _lib.CovSamplingCfg)."""
    arr, n, _keep = _yaml_modules(doc)
    cuts, shadow, motion, cs = _lib.ChainCuts(), _lib.ShadowCfg(), _lib.MotionCfg(), _lib.CovSamplingCfg()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_parts_carried(arr, n, int(carried), C.byref(cuts), C.byref(shadow), C.byref(motion), C.byref(cs),
                                                   why, len(why))
    return rc, why.value.decode(), cuts, shadow, motion, cs


def chain_load_cuts(doc):
    """lsgpu_chain_load_cuts on the same document: the cut modules of its two filter sections -> (return code, reason of a
    refusal, _lib.ChainCuts).  Same rules, same verdict and same text as chain_load."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.ChainCuts()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_cuts(arr, n, C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def chain_load_shadow(doc):
    """lsgpu_chain_load_shadow on the same document: ShadowDataPointsFilter's eps of its two filter sections -> (return code,
    reason of a refusal, _lib.ShadowCfg).  Same rules, same verdict and same text as chain_load."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.ShadowCfg()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_shadow(arr, n, C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def chain_load_cov_sampling(doc):
    """lsgpu_chain_load_cov_sampling on the same document: CovarianceSamplingDataPointsFilter's parameters of its two filter
    sections -> (return code, reason of a refusal, _lib.CovSamplingCfg).  Same rules, same verdict and same text as chain_load."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.CovSamplingCfg()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_cov_sampling(arr, n, C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def chain_load_motion(doc):
    """lsgpu_chain_load_motion on the same document: force2D / force4DOF of PointToPlaneErrorMinimizer and
    BoundTransformationChecker -> (return code, reason of a refusal, _lib.MotionCfg).  Same rules, verdict and text as chain_load."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.MotionCfg()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_motion(arr, n, C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def chain_load_modules(doc, carried: int = 0):
    """lsgpu_chain_load_modules: the whole document in one walk -> (return code, reason of a refusal, _lib.ChainModules): what
    chain_load and the part loaders give, in one record, under the declaration `carried`."""
    arr, n, _keep = _yaml_modules(doc)
    out = _lib.ChainModules()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_modules(arr, n, int(carried), C.byref(out), why, len(why))
    return rc, why.value.decode(), out


def _f32(x) -> float:
    """The shortest decimal that is this float32 (0.75, not 0.75000000000000011...): what the document said."""
    return float(str(np.float32(x)))


def _chain_config(lc, cuts=None, shadow=None, motion=None, cov_sampling=None) -> "ChainConfig":
    """_lib.LoadedChain (and the other parts of the same document's _lib.ChainModules) -> ChainConfig"""
    i, c = lc.icp, lc.chain
    name = {v: k for k, v in _MINIMIZERS.items()}[i.error_minimizer]
    ch = ChainConfig(reading_sampling_prob=_f32(c.reading_prob), surface_normal_knn=c.ssn_knn,
                     surface_normal_ratio=_f32(c.ssn_ratio), reference_normal_knn=c.sn_knn, trim_ratio=_f32(i.trim_ratio),
                     max_iterations=i.max_iterations, min_diff_rot=_f32(i.min_diff_rot), min_diff_trans=_f32(i.min_diff_trans),
                     smooth_length=i.smooth_length, error_minimizer=name, matcher_knn=i.matcher_knn,
                     matcher_max_dist=_f32(i.matcher_max_dist), outlier_max_dist=_f32(i.outlier_max_dist),
                     outlier_min_dist=_f32(i.outlier_min_dist), outlier_median_factor=_f32(i.outlier_median_factor))
    if lc.has_robust:
        r = lc.robust
        word = lambda table, v: next(k for k, x in table.items() if x == v)
        ch.robust = RobustConfig(word(_lib.ROBUST_FCT, r.robust_fct), _f32(r.tuning), word(_lib.ROBUST_SCALE, r.scale_estimator),
                                 r.nb_iteration_for_scale, word(_lib.ROBUST_DIST, r.distance_type), _f32(r.approximation))
    if lc.has_normals:
        n = lc.normals
        ch.normals = NormalsConfig(_f32(n.max_angle), n.reading_sn_knn, n.reading_orient, n.reference_orient,
                                   tuple(_f32(v) for v in n.reading_sensor), tuple(_f32(v) for v in n.reference_sensor),
                                   n.reading_normals_given)
    sd = C.c_float()
    if _lib.lib().lsgpu_loaded_chain_covariance(C.byref(lc), C.byref(sd)):
        ch.covariance = _f32(sd.value)
    md = C.c_float()
    if _lib.lib().lsgpu_loaded_chain_max_density(C.byref(lc), C.byref(md)):
        ch.max_density = float(md.value) if np.isinf(md.value) else _f32(md.value)
    if cuts is not None and (cuts.n_reading or cuts.n_reference):
        ch.cuts = _chain_cuts(cuts)
    if shadow is not None and (shadow.reading_eps >= 0 or shadow.reference_eps >= 0):
        ch.shadow = tuple(_f32(e) if e >= 0 else None for e in (shadow.reading_eps, shadow.reference_eps))
    if motion is not None and (motion.dof or motion.bound):
        ch.motion = _motion_config(motion)
    if cov_sampling is not None and _cov_sampling_pairs(cov_sampling):
        ch.cov_sampling = _cov_sampling_pairs(cov_sampling)
    return ch


class ICP:
    """Drop-in for the reference's ``PointMatcher::ICP icp_`` member."""

    def __init__(self, device: int = 0):
        self.device = device
        self.chain = ChainConfig()
        self._handle: Optional[IcpHandle] = None
        self.last_stats: Optional[IcpStats] = None
        self.carried = 0        # load_from_yaml's declaration: which clouds carry normals (_lib.CARRIED_*)

    # -- laser_track.cpp:20
    def set_default(self):
        self.chain = ChainConfig(reading_sampling_prob=0.75, surface_normal_knn=7,
                                 surface_normal_ratio=0.5, trim_ratio=0.85, max_iterations=40,
                                 min_diff_rot=0.001, min_diff_trans=0.001, smooth_length=3)
        self._handle = None

    # -- laser_track.cpp:17
    def load_from_yaml(self, stream, carried: int = 0):
        """stream: file object, path or YAML text.  Unsupported modules raise (bad config), as
        PointMatcher's registrar does for unknown module names.
        carried: which of compute's clouds carry normals (_lib.CARRIED_READING | _lib.CARRIED_REFERENCE): the chain may then
        read normals without a module that computes them, and compute hands over the normals of the declared sides."""
        import yaml
        if hasattr(stream, "read"):
            text = stream.read()
        else:
            try:
                with open(stream) as f:
                    text = f.read()
            except (OSError, ValueError):
                text = stream
        doc = yaml.load(text, Loader=yaml.BaseLoader)           # scalars stay text: the library reads the numbers
        if doc is None:
            doc = {}
        if not isinstance(doc, dict):
            raise LsgpuError(_lib.BAD_CONFIG, "load_from_yaml", "not a YAML mapping")
        rc, why, loaded = chain_load_modules(doc, carried)
        if rc != _lib.OK:
            raise LsgpuError(_lib.BAD_CONFIG, "load_from_yaml", why)
        self.chain = _chain_config(loaded.chain, loaded.cuts, loaded.shadow, loaded.motion, loaded.cov_sampling)
        self.carried = int(carried)
        self._handle = None

    def _ensure_handle(self) -> IcpHandle:
        if self._handle is None:
            cfg = IcpConfig()
            _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
            cfg.trim_ratio = self.chain.trim_ratio
            cfg.max_iterations = self.chain.max_iterations
            cfg.min_diff_rot = self.chain.min_diff_rot
            cfg.min_diff_trans = self.chain.min_diff_trans
            cfg.smooth_length = self.chain.smooth_length
            self._handle = IcpHandle(cfg, self.device, self.chain.error_minimizer, self.chain.matcher_knn,
                                     self.chain.matcher_max_dist, self.chain.outlier_max_dist,
                                     self.chain.outlier_min_dist, self.chain.outlier_median_factor,
                                     robust=self.chain.robust, normals=self.chain.normals,
                                     covariance=self.chain.covariance, cuts=self.chain.cuts,
                                     max_density=self.chain.max_density, shadow=self.chain.shadow,
                                     motion=self.chain.motion, cov_sampling=self.chain.cov_sampling)
        return self._handle

    @property
    def handle(self) -> IcpHandle:
        """The IcpHandle the chain runs on (created on first use)."""
        return self._ensure_handle()

    def quality(self):
        """IcpHandle.quality() of the last compute (a chain with PointToPlaneWithCovErrorMinimizer)."""
        return self._ensure_handle().quality()

    @property
    def covariance(self) -> np.ndarray:
        """errorMinimizer->getCovariance(): the 6x6 float64 covariance of the last compute.  Raises LsgpuError with the
        library's code before a compute, after a singular H, or on a chain without PointToPlaneWithCovErrorMinimizer."""
        return self.quality()["covariance"]

    # -- laser_track.cpp:496 / incremental_estimator.cpp:108
    def compute(self, reading_xyz1, reference_xyz1, T_init, reading_normals=None, reference_normals=None) -> np.ndarray:
        """T (4x4 float32) with p_reference = T p_reading.  Raises ConvergenceError.
        reading_normals / reference_normals: handed over iff load_from_yaml declared that side as carrying normals."""
        h = self._ensure_handle()
        ch = self.chain
        if not self.carried & _lib.CARRIED_READING:
            reading_normals = None
        if not self.carried & _lib.CARRIED_REFERENCE:
            reference_normals = None
        elif reference_normals is None and h.reads_reference_normals() and not (ch.surface_normal_knn or ch.reference_normal_knn):
            raise LsgpuError(_lib.BAD_CONFIG, "compute", "the chain reads the reference's normals and the reference, declared as "
                             "carrying normals, carries none")
        T, st = h.compute(reading_xyz1, reference_xyz1, T_init, ch.reading_sampling_prob,
                          ch.surface_normal_knn, ch.surface_normal_ratio, ch.seed, ch.reference_normal_knn,
                          reading_normals=reading_normals, reference_normals=reference_normals)
        self.last_stats = st
        return T
