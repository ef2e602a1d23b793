"""RobustOutlierFilter (weighted M-estimator pairs with a MAD scale) through every layer: both YAML loaders, the config
check, the host twins of the scale and the weights, the launch policy, and on the GPU the device loop against a test-side
loop -- brute-force neighbours, the host twins for scale and weights, weighted sums in numpy float64 and the two host solves.

The contract is in include/lsgpu_icp.h ("RobustOutlierFilter"): per iteration scale = sqrt(MAD of the valid d2) (or 1),
e = d2 or (n . (p - q))^2, w = robustFct(e / scale^2, tuning); the weights of all outlier filters multiply, n_used counts
the pairs with w > 0, limit stays the binary filters' upper limit (+inf with none).

Tolerances.  Host twins against the device: bits.  lsgpu_robust_weights against a float64 model: max(1e-6 relative, 1e-6
absolute) -- at most six float roundings per weight, 6 x 2^-24 = 3.6e-7.  w_sum device against numpy: 1e-9 relative (the
weights are the same bits, the sums differ by their order: n x 2^-53 for n <= 8.4 M pairs).  Final T: 1e-5 m / 1e-6 rad,
what tests/test_outlier_chain.py holds its numpy-ordered sums to."""
import ctypes as C
import io
import math
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

import test_outlier_chain as toc
from test_outlier_chain import brute  # noqa: F401  (the exact k-NN fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
FCTS = ["cauchy", "huber", "tukey", "gm", "sc", "L1"]


def robust_yaml(params, before="", after="", p2p=False, reference=True, knn=1):
    y = "readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
    if reference:
        y += "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
    y += f"matcher:\n  KDTreeMatcher:\n    knn: {knn}\n    epsilon: 0\n"
    y += "outlierFilters:\n" + before
    y += "  - RobustOutlierFilter\n" if not params else "  - RobustOutlierFilter:\n" + "".join(f"      {k}: {v}\n" for k, v in params)
    y += after
    y += "errorMinimizer:\n  " + ("PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer") + "\n"
    return y + ("transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
                "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
                "      smoothLength: 4\n")


# ------------------------------------------------------------------------------------------------ CPU

def test_python_loader_reads_the_robust_filter():
    from laser_slam_amd import icp
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(robust_yaml([])))
    assert o.chain.robust == icp.RobustConfig("cauchy", 1.0, "mad", 0, "point2point", math.inf)
    assert o.chain.trim_ratio == 1.0
    allp = [("robustFct", "huber"), ("tuning", 1.5), ("scaleEstimator", "none"), ("nbIterationForScale", 3),
            ("distanceType", "point2plane"), ("approximation", 2.5)]
    o.load_from_yaml(io.StringIO(robust_yaml(allp)))
    assert o.chain.robust == icp.RobustConfig("huber", 1.5, "none", 3, "point2plane", 2.5)
    for f in FCTS:
        o.load_from_yaml(io.StringIO(robust_yaml([("robustFct", f)])))
        assert o.chain.robust.robust_fct == f
        rb = icp.robust_cfg(o.chain.robust)
        assert rb.robust_fct == _lib.ROBUST_FCT[f] and _lib.lib().lsgpu_robust_config_check(C.byref(rb), 0, 1) == _lib.OK
    trim, maxd = "  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n", "  - MaxDistOutlierFilter:\n      maxDist: 0.4\n"
    o.load_from_yaml(io.StringIO(robust_yaml(allp, before=trim, after=maxd)))
    a = o.chain
    o.load_from_yaml(io.StringIO(robust_yaml(allp, after=maxd + trim)))
    assert a == o.chain and a.trim_ratio == 0.8 and a.outlier_max_dist == 0.4 and a.robust.tuning == 1.5
    o.load_from_yaml(io.StringIO(toc.chain_yaml([("trim", 0.75)])))
    assert o.chain.robust is None
    assert icp.ChainConfig().robust is None
    o.load_from_yaml(io.StringIO(robust_yaml([("distanceType", "point2plane")], p2p=True)))      # normals from the filter
    o.load_from_yaml(io.StringIO(robust_yaml([("distanceType", "point2point")], p2p=True, reference=False)))
    bad = [[("robustFct", "welsch")], [("robustFct", "student")], [("scaleEstimator", "berg")], [("scaleEstimator", "std")],
           [("robustFct", "lorentz")], [("scaleEstimator", "iqr")], [("distanceType", "point2line")], [("tuning", -1)],
           [("tuning", ".nan")], [("approximation", -0.5)], [("approximation", ".nan")], [("nbIterationForScale", -1)],
           [("nbIterationForScale", 1.5)], [("ratio", 0.5)]]
    ys = [robust_yaml(p) for p in bad] + [robust_yaml([], after="  - RobustOutlierFilter\n"),
                                          robust_yaml(allp, before="  - RobustOutlierFilter\n"),
                                          robust_yaml([("distanceType", "point2plane")], p2p=True, reference=False)]
    for y in ys:
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(y))
        assert e.value.code == _lib.BAD_CONFIG and "RobustOutlierFilter" in str(e.value), (y, str(e.value))
    for name in ("welsch", "student"):                           # the reason is in the text
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(robust_yaml([("robustFct", name)])))
        assert "exp / pow" in str(e.value)


def test_cpp_loader_reads_the_robust_filter(tmp_path):
    toc._build_cpp(tmp_path, "robust_loader_check")


def test_robust_policy(tmp_path):
    toc._build_cpp(tmp_path, "robust_policy_check", link=False)


def test_shim_and_mirror_compile_with_the_filter(tmp_path):
    """integration/lsgpu_icp_shim.hpp carries the filter from the loader to the handle (compile check, as shim_check)."""
    src = tmp_path / "shim_robust.cpp"
    src.write_text('#include "laser_slam_amd/icp.hpp"\n#include "lsgpu_icp_shim.hpp"\n'
                   'int main() { laser_slam_amd::ICP i; return i.robustFilter() == nullptr ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           str(src)])


def test_config_check_agrees_with_the_loaders():
    L = _lib.lib()

    def fresh(**kw):
        c = _lib.RobustCfg()
        L.lsgpu_robust_config_default(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    d = fresh()
    assert (d.robust_fct, d.tuning, d.scale_estimator, d.nb_iteration_for_scale, d.distance_type) == (0, 1.0, 1, 0, 0)
    assert math.isinf(d.approximation) and d.approximation > 0
    assert L.lsgpu_robust_config_check(C.byref(d), 0, 1) == _lib.OK and L.lsgpu_robust_config_check(C.byref(d), 1, 0) == _lib.OK
    for kw in (dict(robust_fct=6), dict(robust_fct=7), dict(robust_fct=8), dict(scale_estimator=2), dict(scale_estimator=3),
               dict(tuning=-1.0), dict(tuning=float("nan")), dict(approximation=-0.5), dict(approximation=float("nan")),
               dict(nb_iteration_for_scale=-1), dict(distance_type=2)):
        assert L.lsgpu_robust_config_check(C.byref(fresh(**kw)), 0, 1) == _lib.BAD_CONFIG, kw
    plane = fresh(distance_type=1)
    assert L.lsgpu_robust_config_check(C.byref(plane), _lib.MINIMIZER_POINT_TO_POINT, 0) == _lib.BAD_CONFIG
    assert L.lsgpu_robust_config_check(C.byref(plane), _lib.MINIMIZER_POINT_TO_POINT, 1) == _lib.OK
    assert L.lsgpu_robust_config_check(None, 0, 1) == _lib.BAD_CONFIG
    from laser_slam_amd import icp
    for kw in (dict(robust_fct="welsch"), dict(scale_estimator="berg"), dict(tuning=-1.0)):     # before the device is touched
        with pytest.raises(_lib.LsgpuError) as e:
            icp.IcpHandle(robust=kw)
        assert e.value.code == _lib.BAD_CONFIG and "RobustOutlierFilter" in str(e.value)


def test_header_declarations_are_exported_and_the_config_layout_is_unchanged():
    names = ["lsgpu_robust_config_default", "lsgpu_robust_config_check", "lsgpu_icp_set_robust_filter", "lsgpu_robust_scale",
             "lsgpu_robust_weights", "lsgpu_icp_get_robust_trace", "lsgpu_point_to_plane_solve"]
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lsgpu_icp.h")).read()
    for n in names:
        assert hasattr(L, n) and n + "(" in hdr and n in _lib.ABI_SYMBOLS, n
    assert "#define LSGPU_ABI_VERSION 4" in hdr and L.lsgpu_abi_version() == 4
    K = _lib.IcpConfig
    assert C.sizeof(K) == 15 * 4
    fields = ["trim_ratio", "max_iterations", "min_diff_rot", "min_diff_trans", "smooth_length", "cell_size", "profile_kernels",
              "reserved", "error_minimizer", "matcher_knn", "matcher_max_dist", "outlier_max_dist", "outlier_min_dist",
              "outlier_median_factor", "reserved_"]
    assert [getattr(K, n).offset for n in fields] == [4 * i for i in range(15)]
    assert C.sizeof(_lib.RobustCfg) == 32 and C.sizeof(_lib.RobustTrace) == 24


def test_robust_scale_is_numpy_partition():
    from laser_slam_amd import icp
    rng = np.random.default_rng(11)
    cases = []
    for n, share in ((1, 0.0), (2, 0.0), (7, 0.5), (1000, 0.3), (1001, 0.0), (65537, 0.9), (300001, 0.01)):
        d2 = (rng.gamma(2.0, 0.01, n) ** 2).astype(np.float32)
        d2[rng.random(n) < share] = INF
        d2[0] = np.float32(0.01)
        cases.append(d2)
    ties = np.repeat(np.float32([0.25, 0.5, 0.5, 1.0, 4.0]), 40)
    cases += [ties, np.concatenate([ties, np.full(100, INF, np.float32)]), rng.permutation(ties), np.full(9, np.float32(0.3))]
    for d2 in cases:
        v = d2[np.isfinite(d2)]
        m = len(v)
        med = np.partition(v, m // 2)[m // 2]
        mad = np.partition(np.abs(v - med).astype(np.float32), m // 2)[m // 2]
        g_med, g_scale = icp.robust_scale(d2)
        assert g_med.tobytes() == np.float32(med).tobytes() and g_scale.tobytes() == np.sqrt(np.float32(mad)).tobytes(), len(d2)
    with pytest.raises(_lib.ConvergenceError):
        icp.robust_scale(np.full(10, INF, np.float32))


def _model_weights(fct, e, scale, k, approx):
    e2 = e.astype(np.float64) / (float(scale) * float(scale))
    k = float(k)
    k2 = k * k
    with np.errstate(divide="ignore", invalid="ignore"):
        w = {"cauchy": lambda: 1.0 / (1.0 + e2 / k2),
             "huber": lambda: np.where(e2 < k2, 1.0, k / np.sqrt(e2)),
             "tukey": lambda: np.where(e2 < k2, (1.0 - e2 / k2) ** 2, 0.0),
             "gm": lambda: k2 / (k + e2) ** 2,
             "sc": lambda: np.where(e2 > k, 4.0 * k2 / (k + e2) ** 2, 1.0),
             "L1": lambda: 1.0 / np.sqrt(e2)}[fct]()
    if math.isfinite(approx):
        w = np.where(e2 >= approx * approx, 0.0, w)
    return w


def test_robust_weights_against_a_float64_model():
    from laser_slam_amd import icp
    rng = np.random.default_rng(12)
    e = np.concatenate([(rng.gamma(2.0, 0.05, 20000) ** 2), 10.0 ** rng.uniform(-8, 3, 20000)]).astype(np.float32)
    for fct in FCTS:
        for scale, k, approx in ((1.0, 1.0, math.inf), (0.173, 1.5, math.inf), (0.05, 0.75, 3.0), (2.5, 4.685, 10.0)):
            scale, k = np.float32(scale), np.float32(k)
            w = icp.robust_weights(dict(robust_fct=fct, tuning=float(k), approximation=approx), scale, e)
            # (branch decisions are taken on the float e2: the model is given that e2, so only roundings differ)
            e2f = (e / np.float32(scale * scale)).astype(np.float32)
            want = _model_weights(fct, e2f, 1.0, k, approx)
            err = np.abs(w.astype(np.float64) - want)
            assert (err <= np.maximum(1e-6 * np.abs(want), 1e-6)).all(), (fct, float(scale), float(k), err.max())
    # exact at the branch points: e2 == k2, e2 == k, e2 >= approximation^2 (scale 1, values exact in float)
    one = np.float32(1.0)
    for k in (np.float32(2.0), np.float32(0.5)):
        k2 = np.float32(k * k)
        pts = np.float32([k2, np.nextafter(k2, np.float32(0)), np.nextafter(k2, INF), k, np.nextafter(k, np.float32(0)), np.nextafter(k, INF)])
        hub = icp.robust_weights(dict(robust_fct="huber", tuning=float(k)), one, pts)
        # e2 == k2 is not < k2: the second branch, k / sqrtf(e2) (which rounds to 1 at and just above k2)
        assert hub[0] == np.float32(k / np.sqrt(k2)) and hub[1] == 1.0 and hub[2] == np.float32(k / np.sqrt(pts[2]))
        far = icp.robust_weights(dict(robust_fct="huber", tuning=float(k)), one, np.float32([4.0 * k2]))
        assert far[0] == np.float32(0.5)
        tuk = icp.robust_weights(dict(robust_fct="tukey", tuning=float(k)), one, pts)
        assert tuk[0] == 0.0 and tuk[1] > 0.0 and tuk[2] == 0.0
        sc = icp.robust_weights(dict(robust_fct="sc", tuning=float(k)), one, pts)
        assert sc[3] == 1.0 and sc[4] == 1.0 and sc[5] == np.float32(np.float32(4.0) * k2) / np.float32((k + pts[5]) * (k + pts[5]))
    a = np.float32(1.5)
    a2 = np.float32(a * a)
    pts = np.float32([a2, np.nextafter(a2, np.float32(0)), np.nextafter(a2, INF), 100.0])
    for fct in FCTS:
        w = icp.robust_weights(dict(robust_fct=fct, tuning=8.0, approximation=float(a)), one, pts)
        assert w[0] == 0.0 and w[1] > 0.0 and w[2] == 0.0 and w[3] == 0.0, fct
    assert np.isinf(icp.robust_weights(dict(robust_fct="L1"), one, np.float32([0.0])))[0]     # the loop's NO_CONVERGENCE case
    for name in ("welsch", "student"):
        with pytest.raises(_lib.LsgpuError):
            icp.robust_weights(dict(robust_fct=name), one, pts)


def _ne_sums(J, r, w):
    """27 point-to-plane sums (21 upper-tri of sum w J J^T, 6 of -sum w J r) in float64, + sum w, sum w r^2."""
    Jd, rd_, wd = J.astype(np.float64), r.astype(np.float64), w.astype(np.float64)
    A = np.einsum("n,na,nc->ac", wd, Jd, Jd)
    s = np.zeros(29)
    s[:21] = A[np.triu_indices(6)]
    s[21:27] = -np.einsum("n,na,n->a", wd, Jd, rd_)
    s[27] = wd.sum()
    s[28] = (wd * rd_ * rd_).sum()
    return s


def _plane_terms(p, q, n):
    """J = [p x n, n] and r = n . (p - q) in float32, in the kernel's operation order."""
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    J = np.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz], axis=1).astype(np.float32)
    r = ((px - q[:, 0]) * nx + (py - q[:, 1]) * ny) + (pz - q[:, 2]) * nz
    return J, r.astype(np.float32)


def test_point_to_plane_solve_is_the_oracle_step(oracle, pair4k):
    from laser_slam_amd import icp
    rf, rn = oracle.sampling_surface_normal(pair4k["ref"], 10, 1.0, 0)
    q = oracle.transform_points(synth.colmajor(pair4k["T_init"]), pair4k["rd"])
    ids, d2 = oracle.KdTree(rf).nn(q, 16)
    ids, d2 = np.asarray(ids, np.int32), np.asarray(d2, np.float32)
    rc, limit = oracle.trim_limit(d2, 0.75)
    assert rc == 0
    rc, A, b, _x, dT, used = oracle.point_to_plane(q, rf, rn, ids, d2, limit, 1)
    assert rc == 0 and used > 1000
    s = np.zeros(27)
    s[:21] = A[np.triu_indices(6)]
    s[21:] = b
    assert icp.point_to_plane_solve(s).T.ravel().tobytes() == dT.tobytes()
    # ... and from sums built here with unit weights, in the oracle's order of accumulation (sequential, double)
    keep = d2 <= np.float32(limit)
    J, r = _plane_terms(q[keep, :3], rf[ids[keep], :3], rn[ids[keep]])
    s2 = np.zeros(27)
    Jd, rd_ = J.astype(np.float64), r.astype(np.float64)
    iu = np.triu_indices(6)
    s2[:21] = np.add.accumulate(Jd[:, iu[0]] * Jd[:, iu[1]], axis=0)[-1]
    s2[21:] = -np.add.accumulate(Jd * rd_[:, None], axis=0)[-1]
    assert icp.point_to_plane_solve(s2).T.ravel().tobytes() == dT.tobytes()
    with pytest.raises(_lib.ConvergenceError):
        icp.point_to_plane_solve(np.zeros(27))


# ------------------------------------------------------------------------------------------------ the test-side loop

def host_robust_icp(oracle, nn, rd, ref, nrm, T_init, k, chain, rb, p2p=False, mean=None):
    """ICP::compute steps 2-7 with {trim, matcher, max, min, median} as tests/test_outlier_chain.py's loop and, if `rb`, the
    RobustOutlierFilter on top: host twins for scale and weights, weighted sums in numpy float64, the two host solves.
    -> (T, iterations, converged, trace [dict(limit, n_used, median, scale, w_sum, recomputed)], facts) or None."""
    from laser_slam_amd import icp
    ratio, smooth, max_it, lim_rot, lim_trans = chain.get("trim", 1.0), 4, 40, 0.001, 0.01
    if mean is None:
        mean = np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] / len(ref)
    mean = np.asarray(mean, np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T_rm_in = np.asarray(T_init, np.float32).copy()
    T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
    reading = oracle.transform_points(synth.colmajor(T_rm_in), rd)
    T_iter = np.eye(4, dtype=np.float32)
    hist, rot7 = [T_iter.copy()], [np.float32(0)]
    it, converged, trace, facts = 0, False, [], []
    scale, med = np.float32(1.0), np.float32(0.0)
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = nn(ref_c, step, k)
        ids, d2 = toc.mask_matches(ids, d2, chain.get("matcher"))
        idf, df = ids.ravel().copy(), d2.ravel().copy()
        uppers = {}
        if ratio < 1.0:
            rc, trim_lim = oracle.trim_limit(df, ratio)
            if rc != 0:
                return None
            uppers["trim"] = np.float32(trim_lim)
        if chain.get("max"):
            uppers["max"] = toc._sq(chain["max"])
        if chain.get("median"):
            rc, m_ = oracle.trim_limit(df, 0.5)
            uppers["median"] = np.float32(np.float32(chain["median"]) * np.float32(m_))
        limit = min(uppers.values()) if uppers else INF
        keep = (df <= limit) & (idf >= 0)
        if chain.get("min"):
            keep &= df >= toc._sq(chain["min"])
        recomputed, fresh = 0, None
        if rb and rb.get("scale_estimator", "mad") == "mad":
            if not np.isfinite(df).any():
                return None
            fresh = icp.robust_scale(df)
            nb = rb.get("nb_iteration_for_scale", 0)
            if nb == 0 or it + 1 <= nb:
                med, scale = fresh
                recomputed = 1
            if not scale > 0:
                return None
        pf = np.repeat(step, k, axis=0)[keep]
        qf = ref_c[idf[keep], :3]
        J = r = None
        if not p2p or (rb and rb.get("distance_type") == "point2plane"):
            J, r = _plane_terms(pf[:, :3], qf, nrm[idf[keep]])
        if rb:
            e = (r * r).astype(np.float32) if rb.get("distance_type") == "point2plane" else df[keep]
            w = icp.robust_weights(rb, scale, e)
            if not np.isfinite(w).all():
                return None
        else:
            w = np.ones(len(pf), np.float32)
        pos = w > 0
        used = int(pos.sum())
        if used == 0:
            return None
        wd = w[pos].astype(np.float64)
        if p2p:
            pd, qd = pf[pos, :3].astype(np.float64), qf[pos].astype(np.float64)
            ee = (pf[pos, :3] - qf[pos]).astype(np.float64)
            s = np.zeros(29)
            s[0:3] = (wd[:, None] * pd).sum(0)
            s[3:6] = (wd[:, None] * qd).sum(0)
            s[6:15] = np.einsum("n,na,nc->ac", wd, qd, pd).ravel()
            s[27] = wd.sum()
            s[28] = (wd * (ee * ee).sum(1)).sum()
            dT = icp.point_to_point_solve(s)
        else:
            s = _ne_sums(J[pos], r[pos], w[pos])
            dT = icp.point_to_plane_solve(s)
        T_iter = toc._mul4(dT, T_iter)
        trace.append(dict(limit=np.float32(limit), n_used=used, median=np.float32(med), scale=np.float32(scale), w_sum=float(s[27]),
                          recomputed=recomputed))
        facts.append(dict(between=float(((w[pos] > 0) & (w[pos] < 1)).mean()), zeroed=float((w == 0).mean()), kept=int(keep.sum()),
                          fresh_scale=None if fresh is None else np.float32(fresh[1])))
        it += 1
        if it >= max_it:
            break
        rot7.append(abs(np.float32(icp.rotation_distance(T_iter, hist[-1]))))
        hist.append(T_iter.copy())
        n = len(hist)
        if n > smooth:
            rot, trans = np.float32(0), np.float32(0)
            for i in range(n - 1, n - smooth - 1, -1):
                rot = np.float32(rot + rot7[i])
                dx, dy, dz = (hist[i][:3, 3] - hist[i - 1][:3, 3]).astype(np.float32)
                trans = np.float32(trans + abs(np.sqrt(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))))
            rot = np.float32(rot / np.float32(smooth))
            trans = np.float32(trans / np.float32(smooth))
            if rot < np.float32(lim_rot) and trans < np.float32(lim_trans):
                converged = True
                break
    Tmean = np.eye(4, dtype=np.float32)
    Tmean[:3, 3] = mean
    return toc._mul4(Tmean, toc._mul4(T_iter, T_rm_in)), it, converged, trace, facts


def _scene(oracle, pair):
    """pair4k through the two sampling filters, with gross outliers: every seventh reading point is thrown up to a metre
    off -- what a robust filter is for, and what makes the final T depend on it."""
    rf, rn, rd, T_init = toc._inputs(oracle, pair)
    rng = np.random.default_rng(77)
    rd = rd.copy()
    out = np.arange(len(rd)) % 7 == 3
    rd[out, :3] += rng.uniform(-1.0, 1.0, (int(out.sum()), 3)).astype(np.float32)
    return rf, rn, rd, T_init


def R(fct="cauchy", tuning=1.0, est="mad", nb=0, dist="point2point", approx=math.inf):
    return dict(robust_fct=fct, tuning=tuning, scale_estimator=est, nb_iteration_for_scale=nb, distance_type=dist, approximation=approx)


# name -> (k, p2p, chain fields, robust parameters)
CASES = {
    "cauchy": (1, False, {}, R("cauchy", 1.0)),
    "huber": (1, False, {}, R("huber", 1.0)),
    "tukey": (1, False, {}, R("tukey", 3.0)),
    "gm": (1, False, {}, R("gm", 1.0)),
    "sc": (1, False, {}, R("sc", 1.0)),
    "L1": (1, False, {}, R("L1", 1.0)),
    "cauchy-none": (1, False, {}, R("cauchy", 0.1, est="none")),
    "cauchy-nb3": (1, False, {}, R("cauchy", 1.0, nb=3)),
    "cauchy-approx": (1, False, {}, R("cauchy", 1.0, approx=2.0)),
    "cauchy-plane": (1, False, {}, R("cauchy", 1.0, dist="point2plane")),
    "cauchy-p2p": (1, True, {}, R("cauchy", 1.0)),
    "huber-plane-p2p": (1, True, {}, R("huber", 1.0, dist="point2plane")),
    "cauchy-k3": (3, False, {}, R("cauchy", 1.0)),
    "tukey-k3-p2p": (3, True, {}, R("tukey", 3.0)),
    "cauchy+trim": (1, False, dict(trim=0.8), R("cauchy", 1.0)),
    "gm+max": (1, True, dict(max=0.3), R("gm", 1.0)),
}

_host_cache = {}


def _host(oracle, brute, pair4k, name, mean=None):
    key = (name, None if mean is None else tuple(np.asarray(mean, np.float32).tolist()))
    if key not in _host_cache:
        k, p2p, ch, rb = CASES[name]
        rf, rn, rd, T_init = _scene(oracle, pair4k)
        _host_cache[key] = (host_robust_icp(oracle, brute, rd, rf, rn, T_init, k, ch, rb, p2p=p2p, mean=mean),
                            host_robust_icp(oracle, brute, rd, rf, rn, T_init, k, ch, None, p2p=p2p, mean=mean))
    return _host_cache[key]


def _check_not_vacuous(name, with_rb, without):
    assert with_rb is not None and without is not None, name
    T, it, _conv, trace, facts = with_rb
    rb = CASES[name][3]
    for f in facts:
        assert f["between"] >= 0.10, (name, f)                   # real-valued weights, not 0 / 1
    if rb["scale_estimator"] == "mad":
        assert all(t["scale"] != 1.0 and t["scale"] > 0 for t in trace), name
    if rb["nb_iteration_for_scale"] == 3:
        assert it >= 5, (name, it)
        assert [t["recomputed"] for t in trace] == [1, 1, 1] + [0] * (it - 3)
        assert all(t["scale"].tobytes() == trace[2]["scale"].tobytes() for t in trace[3:])
        assert facts[3]["fresh_scale"] != trace[3]["scale"], name   # a fresh MAD in iteration 4 would have differed
    if math.isfinite(rb["approximation"]):
        assert all(f["zeroed"] >= 0.01 for f in facts), (name, [f["zeroed"] for f in facts])
    dt, dr = synth.pose_error(T.astype(np.float64), without[0].astype(np.float64))
    assert dt > 1e-4 or dr > 1e-5, (name, dt, dr)                # ten times the comparison tolerance


@pytest.mark.parametrize("name", list(CASES))
def test_the_robust_cases_are_not_vacuous(oracle, brute, pair4k, name):
    """From the test-side loop alone (CPU): what keeps the GPU comparisons from passing with the filter ignored."""
    _check_not_vacuous(name, *_host(oracle, brute, pair4k, name))


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


def _handle(icp_mod, k, p2p, ch, rb):
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.trim_ratio = ch.get("trim", 1.0)
    mini = "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer"
    return icp_mod.IcpHandle(cfg, 0, mini, matcher_knn=k, robust=rb, **toc._fields(ch))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_loop_matches_the_weighted_reference_loop(icp_mod, oracle, brute, pair4k, name):
    k, p2p, ch, rb = CASES[name]
    rf, rn, rd, T_init = _scene(oracle, pair4k)
    with _handle(icp_mod, k, p2p, ch, rb) as h:                  # a fresh handle, one run
        h.set_reference(rf, rn if (not p2p or rb["distance_type"] == "point2plane") else None)
        Tg, st = h.align(rd, T_init)
        trg, rtg = h.trace(), h.robust_trace()
        mean = h.reference_mean()
    host, plain = _host(oracle, brute, pair4k, name, mean)
    _check_not_vacuous(name, host, plain)
    Th, ith, convh, trh, _facts = host
    for i, (a, b, c) in enumerate(zip(trg, rtg, trh)):
        print(i, "device", a["limit"], a["n_used"], b, "host", c)
    assert len(trg) == len(rtg) == st.iterations
    for i, (a, b, c) in enumerate(zip(trg, rtg, trh)):
        assert np.float32(b["median"]).tobytes() == c["median"].tobytes() and np.float32(b["scale"]).tobytes() == c["scale"].tobytes(), (i, b, c)
        assert int(a["n_used"]) == c["n_used"] and np.float32(a["limit"]).tobytes() == c["limit"].tobytes(), (i, a["n_used"], a["limit"], c)
        assert abs(b["w_sum"] - c["w_sum"]) <= 1e-9 * abs(c["w_sum"]), (i, b["w_sum"], c["w_sum"])
        assert b["recomputed"] == c["recomputed"], (i, b, c)
    assert (st.iterations, st.converged) == (ith, int(convh)), (st.iterations, st.converged, ith, convh)
    assert st.final_n_used == trh[-1]["n_used"]
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    print("pose error", dt, dr)
    assert dt <= 1e-5 and dr <= 1e-6, (dt, dr)


@pytest.mark.gpu
def test_normal_eq_takes_the_device_weights(icp_mod, oracle, brute, pair4k):
    """lsgpu_normal_eq on a handle with a point2plane filter against the host twins fed the same residuals."""
    rf, rn, rd, T_init = _scene(oracle, pair4k)
    rb = R("cauchy", 1.0, dist="point2plane")
    with _handle(icp_mod, 1, False, {}, rb) as h:
        h.set_reference(rf, rn)
        mean = h.reference_mean()
        T = synth.colmajor(T_init).copy()
        T[12:15] -= mean
        ids, d2 = h.knn(rd, T)
        limit = np.float32(np.partition(d2, int(0.9 * len(d2)))[int(0.9 * len(d2))])
        out = np.zeros(29)
        q = np.ascontiguousarray(rd, np.float32)
        rc = _lib.lib().lsgpu_normal_eq(h._h, q.ctypes.data, len(q), T.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data,
                                        d2.ctypes.data, float(limit), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0
    ref_c = rf.copy()
    ref_c[:, :3] -= mean
    p = oracle.transform_points(T, rd)
    keep = d2 <= limit
    J, r = _plane_terms(p[keep, :3], ref_c[ids[keep], :3], rn[ids[keep]])
    _med, scale = icp_mod.robust_scale(d2)
    w = icp_mod.robust_weights(rb, scale, (r * r).astype(np.float32))
    want = _ne_sums(J, r, w)
    assert ((w > 0) & (w < 1)).mean() > 0.5 and scale != 1.0
    err = np.abs(out - want)
    print("normal_eq sums", err.max(), np.abs(want).max())
    assert (err[:27] <= 1e-9 * np.abs(want[:27]).max()).all() and (err[27:] <= 1e-9 * np.abs(want[27:])).all(), (out, want)


@pytest.mark.gpu
def test_yaml_robust_chain_through_compute_and_module_order(icp_mod, pair4k):
    allp = [("robustFct", "cauchy"), ("tuning", 1.0), ("scaleEstimator", "mad")]
    trim, maxd = "  - TrimmedDistOutlierFilter:\n      ratio: 0.9\n", "  - MaxDistOutlierFilter:\n      maxDist: 0.6\n"
    digests = []
    for before, after in ((trim, maxd), ("", maxd + trim), (maxd + trim, "")):
        o = icp_mod.ICP()
        o.load_from_yaml(io.StringIO(robust_yaml(allp, before=before, after=after)))
        o.chain.seed = 4
        T = o.compute(pair4k["rd"], pair4k["ref"], pair4k["T_init"])
        rt = o._handle.robust_trace()
        assert len(rt) == o.last_stats.iterations > 1 and all(0 < t["scale"] != 1.0 and t["w_sum"] < o._handle.trace()[i]["n_used"]
                                                               for i, t in enumerate(rt))
        digests.append(toc._digest(T, o.last_stats, o._handle.trace()) + repr([(t["scale"].tobytes(), t["w_sum"]) for t in rt]))
    assert digests[0] == digests[1] == digests[2]
    o = icp_mod.ICP()                                            # ... and it is not the chain without the filter
    o.load_from_yaml(io.StringIO(toc.chain_yaml([("trim", 0.9), ("max", 0.6)])))
    o.chain.seed = 4
    T0 = o.compute(pair4k["rd"], pair4k["ref"], pair4k["T_init"])
    assert o._handle.robust_trace() == [] and not np.array_equal(T0, T)


@pytest.mark.gpu
def test_align_batch_with_the_filter_is_sequential_align(icp_mod, oracle):
    pairs = toc._batch_pairs(oracle)
    refs, nrms, rds, Tis = map(list, zip(*pairs))
    rb = R("huber", 1.0)
    hs = [_handle(icp_mod, 1, False, dict(trim=0.9), rb) for _ in range(2)]
    Tb, stb, rcb = icp_mod.align_batch(hs, refs, nrms, rds, Tis)
    for h in hs:
        h.close()
    assert list(rcb) == [0] * len(pairs)
    with _handle(icp_mod, 1, False, dict(trim=0.9), rb) as h:
        for i, (rf, rn, rd, Ti) in enumerate(pairs):
            h.set_reference(rf, rn)
            T, st = h.align(rd, Ti)
            assert np.array_equal(T, Tb[i]) and st.iterations == stb[i].iterations and st.iterations > 1
            assert st.final_n_used == stb[i].final_n_used and st.final_limit == stb[i].final_limit


@pytest.mark.gpu
def test_l1_with_a_coincident_pair_is_no_convergence(icp_mod, oracle, pair4k):
    rf, rn, _rd, _Ti = toc._inputs(oracle, pair4k)
    rd = rf[::3].copy()                                          # reading points ON reference points, identity guess: e2 = 0
    with _handle(icp_mod, 1, False, {}, R("L1", 1.0, est="none")) as h:
        h.set_reference(rf, rn)
        Ti = np.ascontiguousarray(np.eye(4, dtype=np.float32).ravel())
        T_out = np.full(16, 7.0, np.float32)
        st = _lib.IcpStats()
        q = np.ascontiguousarray(rd, np.float32)
        rc = _lib.lib().lsgpu_icp_align(h._h, q.ctypes.data, len(q), Ti.ctypes.data_as(C.POINTER(C.c_float)),
                                        T_out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        assert rc == _lib.NO_CONVERGENCE and np.array_equal(T_out, Ti)
        assert "RobustOutlierFilter" in _lib.lib().lsgpu_last_error(h._h).decode()
        h.set_robust_filter(None)                                # the handle works without the filter afterwards
        _T, st2 = h.align(rd, np.eye(4, dtype=np.float32))
        assert st2.iterations >= 1


@pytest.mark.gpu
def test_split_scan_refuses_a_robust_handle(icp_mod, pair4k):
    with icp_mod.IcpHandle(robust=R()) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, icp_mod.comm_unique_id())
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and "RobustOutlierFilter" in str(e.value)
        h.set_reference(pair4k["ref"], None)
        ids, _d2 = h.knn(pair4k["rd"])
        assert len(ids) == len(pair4k["rd"])
    with icp_mod.IcpHandle(error_minimizer="PointToPointErrorMinimizer", robust=R(dist="point2plane")) as h:
        h.set_reference(pair4k["ref"], None)                     # point2plane distances without normals
        with pytest.raises(_lib.LsgpuError) as e:
            h.align(pair4k["rd"], pair4k["T_init"])
        assert e.value.code == _lib.BAD_CONFIG and "point2plane" in str(e.value)
