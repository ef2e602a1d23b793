"""The test-side ICP loop and the exact CPU k-NN it searches with -- shared by tests/test_knn_matcher.py,
tests/test_outlier_chain.py, tests/test_direction_index.py and tests/test_reading_sizes.py (with its worker).  Test
infrastructure only: numpy, the CPU oracle's primitives and the host twins of the solves, no device."""
import ctypes as C
import os
import subprocess

import numpy as np

from laser_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_brute(directory):
    """knn_brute (tests/cpp/knn_brute.c), compiled into `directory`: exact k-NN in the device's arithmetic, 16 threads at
    most.  -> knn(ref_xyz1, q_xyz1, k) -> (ids, d2), each (nq, k), a query's matches in ascending (d2, reference index)."""
    so = os.path.join(str(directory), "libknn_brute.so")
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "knn_brute.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    L.knn_brute.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def knn(ref_xyz1, q_xyz1, k):
        r = np.ascontiguousarray(ref_xyz1, np.float32)
        q = np.ascontiguousarray(q_xyz1, np.float32)
        ids = np.empty((len(q), k), np.int32)
        d2 = np.empty((len(q), k), np.float32)
        assert L.knn_brute(r.ctypes.data, len(r), q.ctypes.data, len(q), k, 16, ids.ctypes.data, d2.ctypes.data) == 0
        return ids, d2
    return knn


def d2_f32(q, p):
    """fma(dz, dz, fma(dy, dy, dx * dx)) in float32, the definition of the device's distances (as _check_nn restates it)."""
    dx, dy, dz = ((q[:, k] - p[:, k]).astype(np.float32) for k in range(3))
    dd = np.float32(dx * dx)
    dd = (dy.astype(np.float64) * dy + dd).astype(np.float32)
    return (dz.astype(np.float64) * dz + dd).astype(np.float32)


def _mul4(a, b):
    """a @ b in float32 with the operation order of hostmath::mul4 / the oracle's mat4_mul (4x4, row-major numpy)."""
    s = a[:, 0:1] * b[0:1, :]
    s = s + a[:, 1:2] * b[1:2, :]
    s = s + a[:, 2:3] * b[2:3, :]
    s = s + a[:, 3:4] * b[3:4, :]
    return s.astype(np.float32)


def _p2p_sums(p, q):
    pd, qd = p.astype(np.float64), q.astype(np.float64)
    e = (p - q).astype(np.float64)
    s = np.zeros(29)
    s[0:3] = pd.sum(0)
    s[3:6] = qd.sum(0)
    s[6:15] = np.einsum("na,nc->ac", qd, pd).ravel()
    s[27] = len(p)
    s[28] = (e * e).sum()
    return s


class _Cfg:
    """icp_default.yaml:14-27 (lsgpu_icp_config_yaml)."""
    trim_ratio, max_iterations, min_diff_rot, min_diff_trans, smooth_length = 0.75, 40, 0.001, 0.01, 4


def host_kmatch_icp(oracle, brute, rd, ref, nrm, T_init, k, p2p=False, mean=None, cfg=_Cfg):
    """ICP::compute steps 2-7 with KDTreeMatcher knn = k: centre the reference on its mean (float of the sequential double
    sum, or `mean`), move the reading by T_refMean_dataIn, then {transform, k-NN, trimmed limit over the k N distances,
    minimizer on the flattened pairs, checkers}.  -> (T 4x4 float32, iterations, converged, [(limit, n_used)])."""
    from laser_slam_amd import icp
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
    it, converged, trace = 0, False, []
    smooth = cfg.smooth_length
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = brute(ref_c, step, k)
        idf, df = ids.ravel(), d2.ravel()                    # Matches, k x N column major, flattened
        rc, limit = oracle.trim_limit(df, cfg.trim_ratio)
        assert rc == 0
        pf = np.repeat(step, k, axis=0)                      # the reading point once per match
        if p2p:
            w = df <= np.float32(limit)
            dT = icp.point_to_point_solve(_p2p_sums(pf[w, :3], ref_c[idf[w], :3]))
            used = int(w.sum())
        else:
            rc, _A, _b, _x, dT16, used = oracle.point_to_plane(pf, ref_c, nrm, idf, df, limit, 1)
            assert rc == 0
            dT = dT16.reshape(4, 4).T
        T_iter = _mul4(dT, T_iter)
        trace.append((np.float32(limit), int(used)))
        it += 1
        if it >= cfg.max_iterations:              # CounterTransformationChecker
            break
        rot7.append(abs(np.float32(icp.rotation_distance(T_iter, hist[-1]))))
        hist.append(T_iter.copy())
        n = len(hist)
        if n > smooth:                            # DifferentialTransformationChecker (float, hostmath::checker_check)
            rot, trans = np.float32(0), np.float32(0)
            for i in range(n - 1, n - smooth - 1, -1):
                rot = np.float32(rot + rot7[i])
                dx, dy, dz = (hist[i][:3, 3] - hist[i - 1][:3, 3]).astype(np.float32)
                trans = np.float32(trans + abs(np.sqrt(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))))
            rot = np.float32(rot / np.float32(smooth))
            trans = np.float32(trans / np.float32(smooth))
            if rot < np.float32(cfg.min_diff_rot) and trans < np.float32(cfg.min_diff_trans):
                converged = True
                break
    Tmean = np.eye(4, dtype=np.float32)
    Tmean[:3, 3] = mean
    return _mul4(Tmean, _mul4(T_iter, T_rm_in)), it, converged, trace
