"""SurfaceNormalOutlierFilter (maxAngle), SurfaceNormalDataPointsFilter on the reading and the orientation pair
(ObservationDirection + OrientNormals): the Python loader, the config check, the host twins, and on the GPU the device loop
against a test-side loop -- brute-force neighbours, the twins for the 0 / 1 angle weights, sums in numpy float64 and the host
solves, in the manner of tests/test_robust_outlier_filter.py.

The contract is in include/lsgpu_icp.h ("SurfaceNormalOutlierFilter"): eps = (float)cos((double)maxAngle); a valid pair is
rejected iff v = normalized(R_iter n0) . normalized(n_ref) < eps, n0 = R_init n_reading; the weights multiply.

Tolerances.  Twins against the device: bits.  lsgpu_normal_angle_weights against a float64 model: exact outside the band
|v64 - cos(maxAngle)| < 1e-5 (three products and two normalisations, each within 2^-24 relative: below 1e-6), the band holds at
most 1 % of the pairs.  Final T: 1e-5 m / 1e-6 rad, what tests/test_outlier_chain.py holds its numpy-ordered sums to.

Shares of the valid pairs the angle test alone rejects in iteration 0 of the GPU cases (test_the_angle_cases_are_not_vacuous
asserts 5 % .. 60 % for each; the figures are printed by that test)."""
import ctypes as C
import io
import math
import os

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

import test_outlier_chain as toc
import test_robust_outlier_filter as tro
from test_outlier_chain import brute  # noqa: F401  (the exact k-NN fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)

SN_RD = "  - SurfaceNormalDataPointsFilter:\n      knn: 7\n"
PAIR_RD = "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n"
PAIR_REF = "  - ObservationDirectionDataPointsFilter:\n      x: 1\n      y: 2\n      z: 3\n  - OrientNormalsDataPointsFilter:\n      towardCenter: 0\n"
RS = "  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
SSN = "  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
SN = "  - SurfaceNormalDataPointsFilter:\n      knn: 5\n"
SNO = "  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.6\n"
TRIM = "  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"


def chain(reading=RS + SN_RD, reference=SSN, outliers=TRIM + SNO, p2p=False, knn=1, max_dist=None):
    y = ("readingDataPointsFilters:\n" + reading) if reading else ""
    y += ("referenceDataPointsFilters:\n" + reference) if reference else ""
    y += f"matcher:\n  KDTreeMatcher:\n    knn: {knn}\n    epsilon: 0\n" + (f"    maxDist: {max_dist}\n" if max_dist else "")
    y += ("outlierFilters:\n" + outliers) if outliers else ""
    y += "errorMinimizer:\n  " + ("PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer") + "\n"
    return y + ("transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
                "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
                "      smoothLength: 4\n")


# ------------------------------------------------------------------------------------------------ CPU

def test_python_loader_reads_the_normal_modules():
    from laser_slam_amd import icp
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(chain()))
    n = o.chain.normals
    assert (n.max_angle, n.reading_sn_knn, n.reading_orient, n.reference_orient) == (0.6, 7, 0, 0)
    assert o.chain.trim_ratio == 0.75 and o.chain.surface_normal_knn == 10 and o.chain.reference_normal_knn == 0
    o.load_from_yaml(io.StringIO(chain(outliers=TRIM + "  - SurfaceNormalOutlierFilter\n")))
    assert o.chain.normals.max_angle == 1.57
    o.load_from_yaml(io.StringIO(chain(reading=RS + SN_RD + PAIR_RD, reference=SN + PAIR_REF, outliers=SNO + TRIM)))
    n = o.chain.normals
    assert (n.reading_orient, n.reference_orient, n.reading_sensor, n.reference_sensor) == (1, 2, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    assert o.chain.reference_normal_knn == 5 and o.chain.surface_normal_knn == 0
    nc = icp.normals_cfg(n)
    L = _lib.lib()
    assert L.lsgpu_normals_config_check(C.byref(nc), 0, 1) == _lib.OK
    assert L.lsgpu_normals_config_check(C.byref(nc), 0, 0) == _lib.BAD_CONFIG     # no reference normals
    o.load_from_yaml(io.StringIO(chain(reading=SN_RD)))                            # no RandomSampling
    assert o.chain.reading_sampling_prob < 0 and o.chain.normals.reading_sn_knn == 7
    o.load_from_yaml(io.StringIO(chain(reading=RS, reference=SSN + PAIR_REF, outliers=TRIM)))   # the reference pair alone
    assert o.chain.normals.reference_orient == 2 and o.chain.normals.max_angle < 0
    o.load_from_yaml(io.StringIO(chain(p2p=True)))                                 # point-to-point with a reference filter
    o.load_from_yaml(io.StringIO(chain(reading=RS, outliers=TRIM)))                # chains without the modules: as before
    assert o.chain.normals is None and o.chain.extra == {}
    bad = {
        "SurfaceNormalDataPointsFilter": [chain(reading=SN_RD + RS), chain(outliers=TRIM), chain(reading=RS + SN_RD + SN_RD),
                                          chain(reference=SSN + SN)],
        "SurfaceNormalOutlierFilter": [chain(reading=RS), chain(reference="", p2p=True), chain(outliers=SNO + SNO),
                                       chain(outliers="  - SurfaceNormalOutlierFilter:\n      maxAngle: 3.2\n"),
                                       chain(outliers="  - SurfaceNormalOutlierFilter:\n      maxAngle: -0.1\n"),
                                       chain(outliers="  - SurfaceNormalOutlierFilter:\n      maxAngle: .nan\n"),
                                       chain(outliers="  - SurfaceNormalOutlierFilter:\n      ratio: 0.5\n")],
        "OrientNormalsDataPointsFilter": [chain(reading=RS + SN_RD + "  - OrientNormalsDataPointsFilter\n"),
                                          chain(reading=RS + PAIR_RD + SN_RD), chain(reading=RS + PAIR_RD, outliers=TRIM),
                                          chain(reference=PAIR_REF + SSN),
                                          chain(reference=SSN + "  - OrientNormalsDataPointsFilter\n  - ObservationDirectionDataPointsFilter\n"),
                                          chain(reference=SSN + "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter:\n      towardCenter: 2\n")],
        "ObservationDirectionDataPointsFilter": [chain(reference=SSN + "  - ObservationDirectionDataPointsFilter\n"),
                                                 chain(reference=SSN + "  - ObservationDirectionDataPointsFilter:\n      w: 1\n  - OrientNormalsDataPointsFilter\n")],
        "GenericDescriptorOutlierFilter": [chain(outliers=TRIM + "  - GenericDescriptorOutlierFilter\n")],
        "VarTrimmedDistOutlierFilter": [chain(outliers="  - VarTrimmedDistOutlierFilter\n")],
    }
    for name, ys in bad.items():
        for y in ys:
            with pytest.raises(_lib.LsgpuError) as e:
                o.load_from_yaml(io.StringIO(y))
            assert e.value.code == _lib.BAD_CONFIG and name in str(e.value), (name, y, str(e.value))
    with pytest.raises(_lib.LsgpuError) as e:                                     # the reason is in the text
        o.load_from_yaml(io.StringIO(chain(reading=SN_RD + RS)))
    assert "gathered through the sampling" in str(e.value)


def test_cpp_loader_reads_the_normal_modules(tmp_path):
    toc._build_cpp(tmp_path, "normal_outlier_loader_check")


def test_normal_outlier_policy(tmp_path):
    toc._build_cpp(tmp_path, "normal_outlier_policy_check", link=False)


def test_shim_and_mirror_compile_with_the_modules(tmp_path):
    """integration/lsgpu_icp_shim.hpp carries lsgpu_normals_config from the loader to the handle (compile check, as shim_check)."""
    import subprocess
    src = tmp_path / "shim_normals.cpp"
    src.write_text('#include "laser_slam_amd/icp.hpp"\n#include "lsgpu_icp_shim.hpp"\n'
                   'int main() { laser_slam_amd::ICP i; return i.normalsConfig() == nullptr ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           str(src)])


def test_config_check_agrees_with_the_loader_and_layouts_are_unchanged():
    from laser_slam_amd import icp
    L = _lib.lib()

    def fresh(**kw):
        c = _lib.NormalsCfg()
        L.lsgpu_normals_config_default(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    d = fresh()
    assert d.max_angle < 0 and (d.reading_sn_knn, d.reading_orient, d.reference_orient, d.reading_normals_given) == (0, 0, 0, 0)
    assert L.lsgpu_normals_config_check(C.byref(d), 0, 1) == _lib.OK and L.lsgpu_normals_config_check(C.byref(d), 1, 0) == _lib.OK
    ok = [dict(max_angle=1.57, reading_sn_knn=5), dict(max_angle=0.0, reading_sn_knn=32, reading_orient=1),
          dict(max_angle=3.1416, reading_sn_knn=3, reference_orient=2), dict(reference_orient=1),
          dict(max_angle=1.0, reading_normals_given=1)]
    for kw in ok:
        assert L.lsgpu_normals_config_check(C.byref(fresh(**kw)), 0, 1) == _lib.OK, kw
    for kw in (dict(max_angle=3.2, reading_sn_knn=5), dict(max_angle=float("nan"), reading_sn_knn=5), dict(max_angle=1.0),
               dict(reading_sn_knn=5), dict(max_angle=1.0, reading_sn_knn=2), dict(max_angle=1.0, reading_sn_knn=33),
               dict(reading_orient=1), dict(max_angle=1.0, reading_sn_knn=5, reading_orient=3), dict(reference_orient=-1)):
        assert L.lsgpu_normals_config_check(C.byref(fresh(**kw)), 0, 1) == _lib.BAD_CONFIG, kw
    for kw in ok[:4]:
        if kw.get("max_angle", -1) >= 0 or kw.get("reference_orient"):
            assert L.lsgpu_normals_config_check(C.byref(fresh(**kw)), 0, 0) == _lib.BAD_CONFIG, kw
    assert L.lsgpu_normals_config_check(None, 0, 1) == _lib.BAD_CONFIG
    with pytest.raises(_lib.LsgpuError) as e:                                     # before the device is touched
        icp.IcpHandle(normals=dict(max_angle=4.0, reading_sn_knn=5))
    assert e.value.code == _lib.BAD_CONFIG and "SurfaceNormalOutlierFilter" in str(e.value)
    names = ["lsgpu_normals_config_default", "lsgpu_normals_config_check", "lsgpu_icp_set_normals", "lsgpu_icp_reading_normals",
             "lsgpu_icp_align_normals", "lsgpu_icp_get_reference_normals", "lsgpu_orient_normals", "lsgpu_normal_angle_weights",
             "lsgpu_icp_get_normal_angle_trace"]
    hdr = open(os.path.join(ROOT, "include", "lsgpu_icp.h")).read()
    for n in names:
        assert hasattr(L, n) and n + "(" in hdr and n in _lib.ABI_SYMBOLS, n
    assert "#define LSGPU_ABI_VERSION 4" in hdr and L.lsgpu_abi_version() == 4
    assert C.sizeof(_lib.IcpConfig) == 15 * 4 and C.sizeof(_lib.ChainCfg) == 24
    assert C.sizeof(_lib.NormalsCfg) == 48 and C.sizeof(_lib.NormalAngleTrace) == 16


def test_orientation_twin_is_the_numpy_restatement(pair4k):
    from laser_slam_amd import icp
    p = pair4k["ref"]
    n = icp.surface_normal(p, 5)
    for sensor, toward in (((0.0, 0.0, 0.0), True), ((1.5, -2.0, 0.25), True), ((1.5, -2.0, 0.25), False)):
        out = icp.orient_normals(p, n, sensor, toward)
        sv = np.asarray(sensor, np.float32)
        o = (sv[None, :] - p[:, :3]).astype(np.float32)
        # s = fma(o.z, n.z, fma(o.y, n.y, o.x n.x)): each fma in float64 (exact product and sum of floats up to one rounding
        # to double, then one to float -- double rounding cannot change a sign, which is all the rule reads)
        s = np.float32(o[:, 0] * n[:, 0])
        s = (o[:, 1].astype(np.float64) * n[:, 1] + s).astype(np.float32)
        s64 = o[:, 2].astype(np.float64) * n[:, 2] + s
        flip = s64 < 0 if toward else s64 > 0
        want = np.where(flip[:, None], -n, n)
        assert out.tobytes() == want.tobytes() and 0.05 < flip.mean() < 0.95
        s2 = np.einsum("ij,ij->i", o.astype(np.float64), out.astype(np.float64))
        assert ((s2 >= -1e-6) if toward else (s2 <= 1e-6)).all()


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    return T


def _v64(T, rn, fn, ids):
    a = rn.astype(np.float64) @ T[:3, :3].astype(np.float64).T
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    f = fn[ids].astype(np.float64)
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    return np.einsum("ij,ij->i", a, f)


def test_angle_weights_against_a_float64_model(oracle, brute, pair4k):
    from laser_slam_amd import icp
    rf, rn, rd, _T_init = toc._inputs(oracle, pair4k)
    rdn = icp.surface_normal(rd, 7)
    T = _rot((0.3, -0.5, 1.0), 0.35).astype(np.float32)
    T[:3, 3] = (0.1, -0.2, 0.05)
    q = oracle.transform_points(synth.colmajor(T), rd)
    ids, _d2 = brute(rf, q, 1)
    ids = ids.ravel()
    v = _v64(T, rdn, rn, ids)
    for max_angle in (0.4, 1.0, 1.57, 2.5):
        w = icp.normal_angle_weights(T, rdn, rn, ids, max_angle)
        band = np.abs(v - math.cos(max_angle)) < 1e-5
        assert band.mean() <= 0.01
        want = (v >= math.cos(max_angle)).astype(np.float32)
        assert np.array_equal(w[~band], want[~band]) and 0.02 < w.mean() < 1.0, (max_angle, w.mean())   # (both outcomes occur)
    # the rotation of T is applied: with the identity instead, the weights differ
    assert not np.array_equal(icp.normal_angle_weights(T, rdn, rn, ids, 0.4), icp.normal_angle_weights(np.eye(4), rdn, rn, ids, 0.4))


def test_angle_weights_known_answers(oracle, pair4k):
    from laser_slam_amd import icp
    rf, rn, _rd, _T = toc._inputs(oracle, pair4k)
    ids = np.arange(len(rf), dtype=np.int32)
    I = np.eye(4, dtype=np.float32)
    assert (icp.normal_angle_weights(I, rn, rn, ids, 1.57) == 1).all()             # equal normals: all kept, at 0 too
    assert (icp.normal_angle_weights(I, rn, rn, ids, 0.0)[np.abs(np.linalg.norm(rn.astype(np.float64), axis=1) - 1) < 1e-9] >= 0).all()
    assert (icp.normal_angle_weights(I, -rn, rn, ids, 1.57) == 0).all()            # negated: all rejected
    # (at 3.1416 eps rounds to -1.0f and an exactly opposite pair may give v one ulp below it: no known answer there)
    ids2 = np.stack([ids, np.full_like(ids, -1)], axis=1)                          # k = 2 with an invalid match
    w2 = icp.normal_angle_weights(I, rn, rn, ids2, 1.57)
    assert (w2[:, 0] == 1).all() and (w2[:, 1] == 0).all()
    z = rn.copy()
    z[0] = 0                                                                       # zero normal: v = 0; kept iff 0 >= eps
    z[1] = np.nan                                                                  # NaN: kept
    assert list(icp.normal_angle_weights(I, z, rn, ids, 1.0)[:2]) == [0.0, 1.0]    # cos 1.0 > 0
    assert list(icp.normal_angle_weights(I, z, rn, ids, 2.0)[:2]) == [1.0, 1.0]    # cos 2.0 < 0
    assert list(icp.normal_angle_weights(I, rn, z, ids, 1.0)[:2]) == [0.0, 1.0]


# ------------------------------------------------------------------------------------------------ the test-side loop

def host_angle_icp(oracle, nn, rd, rdn, ref, nrm, T_init, k, ch, max_angle, rb=None, p2p=False, mean=None):
    """tests/test_robust_outlier_filter.py's loop with SurfaceNormalOutlierFilter on top (max_angle None: without it): the
    reading normals moved once by R_init, then per iteration the twin's 0 / 1 weights multiply the others'.
    -> (T, iterations, converged, trace [dict(limit, n_used, rejected)], first iteration's share rejected) or None."""
    from laser_slam_amd import icp
    ratio, smooth, max_it, lim_rot, lim_trans = ch.get("trim", 1.0), 4, 40, 0.001, 0.01
    if mean is None:
        mean = np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] / len(ref)
    mean = np.asarray(mean, np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T_rm_in = np.asarray(T_init, np.float32).copy()
    T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
    reading = oracle.transform_points(synth.colmajor(T_rm_in), rd)
    R_in = T_rm_in.copy()
    R_in[:3, 3] = 0
    n0 = oracle.transform_points(synth.colmajor(R_in), np.concatenate([rdn, np.ones((len(rdn), 1), np.float32)], axis=1))[:, :3]
    n0 = np.ascontiguousarray(n0, np.float32)
    T_iter = np.eye(4, dtype=np.float32)
    hist, rot7 = [T_iter.copy()], [np.float32(0)]
    it, converged, trace, share0 = 0, False, [], None
    scale, med = np.float32(1.0), np.float32(0.0)
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = nn(ref_c, step, k)
        ids, d2 = toc.mask_matches(ids, d2, ch.get("matcher"))
        idf, df = ids.ravel().copy(), d2.ravel().copy()
        uppers = {}
        if ratio < 1.0:
            rc, trim_lim = oracle.trim_limit(df, ratio)
            if rc != 0:
                return None
            uppers["trim"] = np.float32(trim_lim)
        if ch.get("max"):
            uppers["max"] = toc._sq(ch["max"])
        limit = min(uppers.values()) if uppers else INF
        keep = (df <= limit) & (idf >= 0)
        rejected = 0
        if max_angle is not None:
            wa = icp.normal_angle_weights(T_iter, n0, nrm, ids.reshape(len(rd), k), max_angle).ravel()
            rejected = int((keep & (wa == 0)).sum())
            if it == 0:
                share0 = float(((idf >= 0) & (wa == 0)).sum() / max(1, (idf >= 0).sum()))
            keep &= wa > 0
        if rb and rb.get("scale_estimator", "mad") == "mad":
            if not np.isfinite(df).any():
                return None
            med, scale = icp.robust_scale(df)
            if not scale > 0:
                return None
        pf = np.repeat(step, k, axis=0)[keep]
        qf = ref_c[idf[keep], :3]
        J = r = None
        if not p2p:
            J, r = tro._plane_terms(pf[:, :3], qf, nrm[idf[keep]])
        w = icp.robust_weights(rb, scale, df[keep]) if rb else np.ones(len(pf), np.float32)
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
            dT = icp.point_to_plane_solve(tro._ne_sums(J[pos], r[pos], w[pos]))
        T_iter = toc._mul4(dT, T_iter)
        trace.append(dict(limit=np.float32(limit), n_used=used, rejected=rejected))
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
    return toc._mul4(Tmean, toc._mul4(T_iter, T_rm_in)), it, converged, trace, share0


def _scene(oracle, pair, cut=None):
    """pair4k through the two sampling filters; normals of both clouds oriented towards the sensor at the origin of the
    frame each was given in.  cut: the reading cut to a length that is no multiple of 64 or 256."""
    from laser_slam_amd import icp
    rf, rn, rd, T_init = toc._inputs(oracle, pair)
    if cut:
        rd = np.ascontiguousarray(rd[:cut])
    rdn = icp.orient_normals(rd, icp.surface_normal(rd, 7), (0, 0, 0))
    rn = icp.orient_normals(rf, rn, (0, 0, 0))
    return rf, rn, rd, rdn, T_init


def _turned(T_init, angle=0.3):
    return (_rot((0, 0, 1), angle) @ np.asarray(T_init, np.float64)).astype(np.float32)


# name -> (k, p2p, sn reference filter, chain fields, robust, maxAngle, turn the guess, reading cut)
# shares rejected by the angle test alone in iteration 0 (printed by the non-vacuity test): plane-k1-trim 0.446, k3 0.425,
# p2p-sn-reference 0.408, matcher-maxdist 0.408, robust-cauchy-mad 0.429, turned-guess 0.487
CASES = {
    "plane-k1-trim": (1, False, False, dict(trim=0.75), None, 0.5, False, 1901),
    "k3": (3, False, False, dict(trim=0.75), None, 0.5, False, None),
    "p2p-sn-reference": (1, True, True, dict(trim=0.75), None, 0.5, False, None),
    "matcher-maxdist": (1, False, False, dict(trim=0.9, matcher=0.5), None, 0.5, False, None),
    "robust-cauchy-mad": (1, False, False, {}, tro.R("cauchy", 1.0), 0.5, False, None),
    "turned-guess": (1, False, False, dict(trim=0.75), None, 0.5, True, None),
}
_cache = {}


def _case(oracle, pair4k, name):
    from laser_slam_amd import icp
    k, p2p, sn_ref, ch, rb, ang, turn, cut = CASES[name]
    rf, rn, rd, rdn, T_init = _scene(oracle, pair4k, cut)
    if sn_ref:                                                   # SurfaceNormalDataPointsFilter's normals on the same points
        rn = icp.orient_normals(rf, icp.surface_normal(rf, 5), (0, 0, 0))
    return rf, rn, rd, rdn, (_turned(T_init) if turn else T_init)


def _host(oracle, brute, pair4k, name, mean=None):
    key = (name, None if mean is None else tuple(np.asarray(mean, np.float32).tolist()))
    if key not in _cache:
        k, p2p, _sn, ch, rb, ang, _turn, _cut = CASES[name]
        rf, rn, rd, rdn, T_init = _case(oracle, pair4k, name)
        _cache[key] = (host_angle_icp(oracle, brute, rd, rdn, rf, rn, T_init, k, ch, ang, rb, p2p, mean),
                       host_angle_icp(oracle, brute, rd, rdn, rf, rn, T_init, k, ch, None, rb, p2p, mean))
    return _cache[key]


def _check_not_vacuous(name, with_a, without):
    assert with_a is not None and without is not None, name
    print(name, "share rejected in iteration 0:", with_a[4])
    assert 0.05 <= with_a[4] <= 0.60, (name, with_a[4])
    assert all(t["rejected"] > 0 for t in with_a[3])
    if CASES[name][3].get("matcher"):
        assert with_a[3][0]["n_used"] > 0


@pytest.mark.parametrize("name", list(CASES))
def test_the_angle_cases_are_not_vacuous(oracle, brute, pair4k, name):
    """From the test-side loop alone (CPU): in iteration 0 the angle test on its own rejects 5 % .. 60 % of the valid pairs."""
    _check_not_vacuous(name, *_host(oracle, brute, pair4k, name))


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


def _handle(icp_mod, k, p2p, ch, rb, ang):
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.trim_ratio = ch.get("trim", 1.0)
    mini = "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer"
    normals = None if ang is None else dict(max_angle=ang, reading_normals_given=1)
    return icp_mod.IcpHandle(cfg, 0, mini, matcher_knn=k, robust=rb, normals=normals, **toc._fields(ch))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_device_loop_matches_the_angle_reference_loop(icp_mod, oracle, brute, pair4k, name):
    k, p2p, _sn, ch, rb, ang, _turn, _cut = CASES[name]
    rf, rn, rd, rdn, T_init = _case(oracle, pair4k, name)
    assert len(rd) % 64 and len(rd) % 256
    with _handle(icp_mod, k, p2p, ch, rb, ang) as h:
        h.set_reference(rf, rn)
        Tg, st = h.align_normals(rd, rdn, T_init)
        trg, nag = h.trace(), h.normal_angle_trace()
        mean = h.reference_mean()
    host, plain = _host(oracle, brute, pair4k, name, mean)
    _check_not_vacuous(name, host, plain)
    Th, ith, convh, trh, _share = host
    for i, (a, b, c) in enumerate(zip(trg, nag, trh)):
        print(i, "device", a["limit"], a["n_used"], b, "host", c)
    assert len(trg) == len(nag) == st.iterations
    for i, (a, b, c) in enumerate(zip(trg, nag, trh)):
        assert int(a["n_used"]) == c["n_used"] and np.float32(a["limit"]).tobytes() == c["limit"].tobytes(), (i, a["n_used"], a["limit"], c)
        assert b["rejected"] == c["rejected"] and b["eps"].tobytes() == np.float32(math.cos(ang)).tobytes(), (i, b, c)
    assert (st.iterations, st.converged) == (ith, int(convh)), (st.iterations, st.converged, ith, convh)
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    print("pose error", dt, dr)
    assert dt <= 1e-5 and dr <= 1e-6, (dt, dr)
    dt0, dr0 = synth.pose_error(Th.astype(np.float64), plain[0].astype(np.float64))   # ... and the filter matters
    assert dt0 > 1e-4 or dr0 > 1e-5 or [t["n_used"] for t in trh] != [t["n_used"] for t in plain[3]]


def _digest(T, st, tr):
    return (np.ascontiguousarray(T).tobytes(), st.iterations, st.converged, st.final_n_used,
            [(np.float32(t["limit"]).tobytes(), int(t["n_used"]), np.asarray(t["T_iter"], np.float32).tobytes()) for t in tr])


@pytest.mark.gpu
def test_inert_cases_are_bit_identical_to_the_plain_chain(icp_mod, oracle, brute, pair4k):
    rf, rn, rd, rdn, T_init = _scene(oracle, pair4k)
    ch = dict(trim=0.75)
    with _handle(icp_mod, 1, False, ch, None, None) as h:        # the chain without the filter (the chain plan: trim + max)
        h0 = icp_mod.IcpHandle(h.cfg, 0, outlier_max_dist=50.0)
        h0.set_reference(rf, rn)
        T0, st0 = h0.align(rd, T_init)
        tr0 = h0.trace()
        d0 = _digest(T0, st0, tr0)
        h0.set_reference(rf, -rn)                                # every reference normal flipped: r and J negate exactly
        T1, st1 = h0.align(rd, T_init)
        tr1 = h0.trace()
        assert _digest(T1, st1, tr1) == d0
        assert all(np.array_equal(a["A"], b["A"]) and np.array_equal(a["b"], b["b"]) for a, b in zip(tr0, tr1))
        h0.close()
    # maxAngle pi on oriented clouds rejects nothing (no pair's v is below -1 + 1e-6 ... as the twin says first)
    ids, _d2 = brute(rf, oracle.transform_points(synth.colmajor(T_init), rd), 1)
    v = _v64(np.asarray(T_init, np.float32), rdn, rn, ids.ravel())
    assert (v >= -1 + 1e-6).all()
    with _handle(icp_mod, 1, False, dict(trim=0.75, max=50.0), None, 3.1416) as h:
        h.set_reference(rf, rn)
        T2, st2 = h.align_normals(rd, rdn, T_init)
        assert _digest(T2, st2, h.trace()) == d0
        assert [t["rejected"] for t in h.normal_angle_trace()] == [0] * st2.iterations
        h.set_normals(dict(max_angle=0.5, reading_normals_given=1))
        T3, st3 = h.align(rd, T_init)                            # plain align: no reading normals, the filter is inert
        assert _digest(T3, st3, h.trace()) == d0 and h.normal_angle_trace() == []
        T4, st4 = h.align_normals(rd, rdn, T_init)               # ... and it is not when they are there
        assert _digest(T4, st4, h.trace()) != d0
    with _handle(icp_mod, 1, True, dict(trim=0.75, max=50.0), None, 0.5) as h:   # a point-to-point reference without normals
        h.set_reference(rf, None)
        T5, st5 = h.align_normals(rd, rdn, T_init)
        h.set_normals(None)
        T6, st6 = h.align(rd, T_init)
        assert np.array_equal(T5, T6) and st5.iterations == st6.iterations and st5.final_n_used == st6.final_n_used


@pytest.mark.gpu
def test_all_pairs_rejected_is_no_convergence(icp_mod, oracle, pair4k):
    rf, rn, rd, rdn, T_init = _scene(oracle, pair4k)
    with _handle(icp_mod, 1, False, dict(trim=0.75), None, 1.57) as h:
        h.set_reference(rf, rn)
        anti = np.zeros((len(rd), 3), np.float32)                # zero reading normals: v = 0 < cos(1.0) for every pair
        h.set_normals(dict(max_angle=1.0, reading_normals_given=1))
        Ti = np.ascontiguousarray(synth.colmajor(T_init), np.float32)
        T_out = np.full(16, 7.0, np.float32)
        st = _lib.IcpStats()
        q = np.ascontiguousarray(rd, np.float32)
        rc = _lib.lib().lsgpu_icp_align_normals(h._h, q.ctypes.data, len(q), anti.ctypes.data, Ti.ctypes.data_as(C.POINTER(C.c_float)),
                                                T_out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        assert rc == _lib.NO_CONVERGENCE and np.array_equal(T_out, Ti)


@pytest.mark.gpu
def test_split_scan_refuses_the_handle(icp_mod):
    with icp_mod.IcpHandle(normals=dict(max_angle=1.0, reading_normals_given=1)) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, icp_mod.comm_unique_id())
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and "SurfaceNormalOutlierFilter" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("knn", [5, 10])
def test_reading_normals_are_the_host_filter_and_leave_the_reference(icp_mod, oracle, pair4k, knn):
    rf, rn, rd, _rdn, _T = _scene(oracle, pair4k, 1901)
    with icp_mod.IcpHandle() as h:
        h.set_reference(rf, rn)
        ids0, d0 = h.knn(rd)
        got = h.reading_normals(rd, knn)
        assert got.tobytes() == icp_mod.surface_normal(rd, knn).tobytes()
        for sensor, mode in (((0.0, 0.0, 0.0), 1), ((1.0, 2.0, 0.5), 2)):
            go = h.reading_normals(rd, knn, mode, sensor)
            assert go.tobytes() == icp_mod.orient_normals(rd, got, sensor, mode == 1).tobytes() and go.tobytes() != got.tobytes()
        ids1, d1 = h.knn(rd)
        assert np.array_equal(ids0, ids1) and np.array_equal(d0, d1)
        assert h.reference_normals().tobytes() == rn.tobytes()


# the end-to-end chains: the reference's sensor a little off the reading's, both clouds oriented towards their sensor (normals
# turned AWAY from a sensor on one side alone face the other side's: the angle test then keeps too few pairs to solve with)
SENSOR_E2E = (0.5, -0.3, 0.2)
PAIR_REF_E2E = ("  - ObservationDirectionDataPointsFilter:\n      x: 0.5\n      y: -0.3\n      z: 0.2\n"
                "  - OrientNormalsDataPointsFilter:\n      towardCenter: 1\n")


def _by_hand(icp_mod, pair, seed, rd_knn, sn_ref, orient, ang, sensor_ref=SENSOR_E2E, toward_ref=True):
    """The kernel-level calls of the chain TRIM 0.75 + SurfaceNormalOutlierFilter: filters with the same seed, normals by the
    twins, set_reference, align_normals."""
    with icp_mod.IcpHandle() as hf:
        if sn_ref:
            rf, rn = np.ascontiguousarray(pair["ref"], np.float32), icp_mod.surface_normal(pair["ref"], 5)
            rd = hf.filter_reading(pair["rd"], 0.5, seed)
        else:
            rf, rn = hf.filter_reference(pair["ref"], 10, 0.5, seed)
            rd = hf.filter_reading(pair["rd"], 0.5, -1)
    rdn = icp_mod.surface_normal(rd, rd_knn)
    if orient:
        rdn = icp_mod.orient_normals(rd, rdn, (0, 0, 0), True)
        rn = icp_mod.orient_normals(rf, rn, sensor_ref, toward_ref)
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    normals = None if ang is None else dict(max_angle=ang, reading_normals_given=1)
    with icp_mod.IcpHandle(cfg, 0, normals=normals, outlier_max_dist=None if ang is not None else 50.0) as h:
        h.set_reference(rf, rn)
        T, st = h.align_normals(rd, rdn, pair["T_init"]) if ang is not None else h.align(rd, pair["T_init"])
        return T, st, h.trace(), rn


@pytest.mark.gpu
@pytest.mark.parametrize("sn_ref", [False, True])
def test_yaml_chain_end_to_end_is_the_calls_by_hand(icp_mod, pair4k, sn_ref):
    y = chain(reading=RS + SN_RD + PAIR_RD, reference=(SN if sn_ref else SSN) + PAIR_REF_E2E)
    o = icp_mod.ICP()
    o.load_from_yaml(io.StringIO(y))
    o.chain.seed = 4
    T = o.compute(pair4k["rd"], pair4k["ref"], pair4k["T_init"])
    st, tr, na = o.last_stats, o._handle.trace(), o._handle.normal_angle_trace()
    nrm_dev = o._handle.reference_normals()
    Th, sth, trh, rn = _by_hand(icp_mod, pair4k, 4, 7, sn_ref, True, 0.6)
    assert nrm_dev.tobytes() == rn.tobytes()                      # the device orientation of the reference is the twin's
    assert _digest(T, st, tr) == _digest(Th, sth, trh)
    assert len(na) == st.iterations > 1 and all(t["rejected"] > 0 for t in na)
    # through resident clouds
    h = o._handle
    h.cloud_upload(0, pair4k["rd"])
    h.cloud_upload(1, pair4k["ref"])
    ch = o.chain
    Tc, stc = h.compute_clouds(0, [1], None, pair4k["T_init"], ch.reading_sampling_prob, ch.surface_normal_knn,
                               ch.surface_normal_ratio, 4, ch.reference_normal_knn)
    assert _digest(Tc, stc, h.trace()) == _digest(Th, sth, trh)


@pytest.mark.gpu
@pytest.mark.parametrize("sn_ref", [False, True])
def test_reference_orientation_alone_changes_nothing(icp_mod, pair4k, sn_ref):
    """Point-to-plane sums do not see the sign of a reference normal: the chain with the reference pair and no angle filter is
    the chain without the pair, bit for bit."""
    digests = []
    for pair in (PAIR_REF, ""):
        o = icp_mod.ICP()
        o.load_from_yaml(io.StringIO(chain(reading=RS, reference=(SN if sn_ref else SSN) + pair,
                                           outliers=TRIM + "  - MaxDistOutlierFilter:\n      maxDist: 50\n")))
        o.chain.seed = 4
        T = o.compute(pair4k["rd"], pair4k["ref"], pair4k["T_init"])
        digests.append(_digest(T, o.last_stats, o._handle.trace()))
        nrm = o._handle.reference_normals()
        if pair:
            flipped = nrm
        else:
            assert 0.05 < (np.abs(flipped + nrm).max(axis=1) == 0).mean() < 0.95   # the pair did flip a share of them
            # ... exactly those the twin flips (towardCenter 0, sensor (1, 2, 3)), on the points the filter kept
            if sn_ref:
                pts = np.ascontiguousarray(pair4k["ref"], np.float32)
            else:
                with icp_mod.IcpHandle() as hf:
                    pts, n_plain = hf.filter_reference(pair4k["ref"], 10, 0.5, 4)
                assert n_plain.tobytes() == nrm.tobytes()
            assert icp_mod.orient_normals(pts, nrm, (1.0, 2.0, 3.0), False).tobytes() == flipped.tobytes()
    assert digests[0] == digests[1]
