"""What tests/test_constrained_step.py shares between its cases: the YAML documents of the loader tests, the float64
restatement of the constrained point-to-plane steps (PointToPlaneErrorMinimizer force2D / force4DOF) and of
BoundTransformationChecker, and the host-side rebuild of a device trace.  Test infrastructure only: numpy, the CPU oracle's
primitives and the library's host twins, no device."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

F = np.float32
INF = F(np.inf)
DOF_6, DOF_3, DOF_4 = 0, 3, 4                      # _lib.MOTION_DOF_*: the free step, force2D, force4DOF
ROWS = {DOF_3: (2, 3, 4), DOF_4: (2, 3, 4, 5)}     # the unknowns of the constrained steps: rows / columns of the 6x6 system

SSN = "  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
TRIM = "  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"
MAXD = "  - MaxDistOutlierFilter:\n      maxDist: 2.0\n"
MIND = "  - MinDistOutlierFilter:\n      minDist: 0.001\n"
MEDIAN = "  - MedianDistOutlierFilter:\n      factor: 3\n"
ROBUST = "  - RobustOutlierFilter:\n      robustFct: cauchy\n      tuning: 1.0\n"
SNO = "  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.6\n"
SN_RD = "  - SurfaceNormalDataPointsFilter:\n      knn: 7\n"
COUNTER = "  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
DIFF = "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 4\n"


def bound(rot=None, trans=None):
    if rot is None and trans is None:
        return "  - BoundTransformationChecker\n"
    y = "  - BoundTransformationChecker:\n"
    y += ("      maxRotationNorm: %s\n" % rot) if rot is not None else ""
    y += ("      maxTranslationNorm: %s\n" % trans) if trans is not None else ""
    return y


def minimizer(name="PointToPlaneErrorMinimizer", **params):
    if not params:
        return "  " + name + "\n"
    return "  " + name + ":\n" + "".join("    %s: %s\n" % kv for kv in params.items())


def chain(mini=None, outliers=TRIM, checkers=COUNTER + DIFF, knn=1, max_dist=None, reading="", reference=SSN):
    y = ("readingDataPointsFilters:\n" + reading) if reading else ""
    y += ("referenceDataPointsFilters:\n" + reference) if reference else ""
    y += "matcher:\n  KDTreeMatcher:\n    knn: %d\n    epsilon: 0\n" % knn + ("    maxDist: %s\n" % max_dist if max_dist else "")
    y += ("outlierFilters:\n" + outliers) if outliers else ""
    y += "errorMinimizer:\n" + (mini if mini is not None else minimizer())
    return y + "transformationCheckers:\n" + checkers


# ------------------------------------------------------------------------------------------------ the float64 restatement

def unpack(sums):
    """27 sums (21 upper-triangular entries of A row major, 6 of b) -> (A 6x6, b 6), float64"""
    s = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27].copy()


def pack(A, b):
    return np.concatenate([np.asarray(A, np.float64)[np.triu_indices(6)], np.asarray(b, np.float64)])


def np_step(sums, dof):
    """The step restated in float64: the sub-system of ROWS[dof] solved with numpy, x = {0, 0, yaw, tx, ty, tz}, dT the
    rotation by yaw about z plus the translation.  dof 0: the free step (AngleAxis of x[:3]).  -> (x 6, dT 4x4)"""
    A, b = unpack(sums)
    x = np.zeros(6)
    dT = np.eye(4)
    if dof == DOF_6:
        x = np.linalg.solve(A, b)
        w = x[:3]
        ang = np.linalg.norm(w)
        if ang > 0:
            k = w / ang
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            dT[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    else:
        r = list(ROWS[dof])
        x[r] = np.linalg.solve(A[np.ix_(r, r)], b[r])
        c, s = np.cos(x[2]), np.sin(x[2])
        dT[:2, :2] = [[c, -s], [s, c]]
    dT[:3, 3] = x[3:6]
    return x, dT


def pair_sums(p, q, n, dof):
    """The 27 sums of the kept pairs (p: reading points at T_iter, q: their matches, n: the matches' normals; float32 rows):
    f = [p x n; n] and the residual in float32 with one rounding per operation, as the device forms them, the products and
    the sums in float64.  force2D (DOF_3): b with the planar residual e2.  -> (27 sums, count)"""
    p, q, n = (np.asarray(a, F)[:, :3] for a in (p, q, n))
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    J = np.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz], 1)
    assert J.dtype == F
    dx, dy, dz = px - q[:, 0], py - q[:, 1], pz - q[:, 2]
    e2 = dx * nx + dy * ny
    e = e2 + dz * nz
    assert e.dtype == F
    eb = (e2 if dof == DOF_3 else e).astype(np.float64)
    Jd = J.astype(np.float64)
    return pack(Jd.T @ Jd, -(Jd * eb[:, None]).sum(0)), len(p)


def np_bound_first_violation(Ts, max_rot, max_trans):
    """BoundTransformationChecker restated in float64: rotation angle of R_i R_0^T, |t_i - t_0|; compared with >"""
    Ts = [np.asarray(T, np.float64) for T in Ts]
    for i in range(1, len(Ts)):
        R = Ts[i][:3, :3] @ Ts[0][:3, :3].T
        ang = np.arctan2(np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2, (np.trace(R) - 1) / 2)
        if ang > max_rot or np.linalg.norm(Ts[i][:3, 3] - Ts[0][:3, 3]) > max_trans:
            return i
    return -1


# ------------------------------------------------------------------------------------------------ the device trace, rebuilt

def mul4(a, b):
    """a @ b in float32 with the operation order of hostmath::mul4 (4x4, row-major numpy)."""
    s = a[:, 0:1] * b[0:1, :]
    s = s + a[:, 1:2] * b[1:2, :]
    s = s + a[:, 2:3] * b[2:3, :]
    s = s + a[:, 3:4] * b[3:4, :]
    return s.astype(F)


def _sq(v):
    return F(F(v) * F(v))


def rebuild_record(prims, reading, ref_c, nrm, T_prev, ch, dof):
    """One iteration of the loop rebuilt at T_prev (4x4 float32): the reading moved by T_prev, its exact neighbours,
    KDTreeMatcher maxDist, the smallest of the upper thresholds {trim, max, median}, MinDist, and the sums of the kept pairs
    (pair_sums, on the host).  `prims`: an object with the kernel-level entries transform_points(T16, pts), knn(pts) (ids
    into the reference as given, squared distances) and trim_limit(d2, ratio) (+inf = an invalid match) -- a plain IcpHandle
    on the same reference, or the CPU oracle's.  `ch`: {"trim", "matcher", "max", "min", "median"}, absent: no such module
    (the rules of tests/test_outlier_chain.py::host_chain_icp, knn 1).  -> (limit float32, n_used, 27 sums)"""
    from laser_slam_amd import synth
    step = prims.transform_points(synth.colmajor(T_prev), reading)
    ids, d2 = prims.knn(step)
    ids, d2 = np.asarray(ids).ravel().copy(), np.asarray(d2, F).ravel().copy()
    if ch.get("matcher"):
        out = ~(d2 <= _sq(ch["matcher"]))
        ids[out] = -1
        d2[out] = INF
    limit = F(prims.trim_limit(d2, ch.get("trim", 1.0)))
    if ch.get("max"):
        limit = min(limit, _sq(ch["max"]))
    if ch.get("median"):
        limit = min(limit, F(F(ch["median"]) * F(prims.trim_limit(d2, 0.5))))
    if ch.get("min"):
        low = np.isfinite(d2) & (d2 < _sq(ch["min"]))
        ids[low] = -1
        d2[low] = INF
    w = (d2 <= limit) & (ids >= 0)
    sums, used = pair_sums(step[w], ref_c[ids[w]], nrm[ids[w]], dof)
    return F(limit), used, sums


def raw_align(h, rd, T_init):
    """lsgpu_icp_align without the facade's exception -> (rc, T_out 4x4 float32, IcpStats, lsgpu_last_error)"""
    from laser_slam_amd import _lib, icp
    p = np.ascontiguousarray(rd, F)
    ti = icp._t16(T_init)
    to = np.full(16, np.nan, F)
    st = icp.IcpStats()
    rc = _lib.lib().lsgpu_icp_align(h._h, p.ctypes.data, len(p), icp._fp(ti), icp._fp(to), C.byref(st))
    return rc, to.reshape(4, 4).T.copy(), st, _lib.lib().lsgpu_last_error(h._h).decode()


def trace_bytes(tr):
    out = b""
    for t in tr:
        out += np.ascontiguousarray(t["T_iter"]).tobytes() + F(t["limit"]).tobytes() + np.int64(t["n_used"]).tobytes()
        out += np.ascontiguousarray(t["A"]).tobytes() + np.ascontiguousarray(t["b"]).tobytes() + np.ascontiguousarray(t["x"]).tobytes()
    return out
