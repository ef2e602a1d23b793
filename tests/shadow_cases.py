"""What tests/test_shadow_filter.py shares between its cases, and (run as a program) the worker of its side-stream case.

The identity under test: ICP.compute on a loaded document with ShadowDataPointsFilter (route a) equals the same compute
assembled by hand (route b) -- the section's other modules by the library's kernel-level entries on the device, the module
itself by its HOST twin (lsgpu_filter_shadow), then set_reference + align / align_normals on a handle that has never heard
of the module: T_out, the result fields of the stats, the trace records and the position of the library's draw stream, bit
for bit.  Timings and the launch policy's counters are not results and are not compared (as in tests/chain_cuts_cases.py)."""
import ctypes as C
import hashlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

SEED = 4
RS = "  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
SN_RD = "  - SurfaceNormalDataPointsFilter:\n      knn: 7\n"
PAIR_RD = "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n"
PAIR_REF = ("  - ObservationDirectionDataPointsFilter:\n      x: 0.5\n      y: -0.3\n      z: 0.2\n"
            "  - OrientNormalsDataPointsFilter:\n      towardCenter: 1\n")
SSN = "  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
SN = "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n"
SN_DENS = "  - SurfaceNormalDataPointsFilter:\n      knn: 10\n      keepDensities: 1\n"
TRIM = "  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"
SNO = "  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.6\n"


def shadow(eps="0.1"):
    return "  - ShadowDataPointsFilter:\n      eps: %s\n" % eps


def max_density(md):
    return "  - MaxDensityDataPointsFilter:\n      maxDensity: %s\n" % md


def chain(reading=RS, reference=SSN, outliers=TRIM, minimizer="PointToPlaneErrorMinimizer"):
    y = ("readingDataPointsFilters:\n" + reading) if reading else ""
    y += ("referenceDataPointsFilters:\n" + reference) if reference else ""
    y += "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n"
    y += ("outlierFilters:\n" + outliers) if outliers else ""
    y += "errorMinimizer:\n  " + minimizer + "\n"
    return y + ("transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
                "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 4\n")


# The cases of the compute test on the 4 k-point pair, seed 4, eps 0.1 everywhere (chosen with the host twins on the CPU; the
# counts are asserted in the test).  Points the module drops / is handed:
#   sampling              reference 326 of 2026
#   surface_normal        reference 1966 of 4096 (the synthetic scan's rings: collinear neighbourhoods, normals across the ray)
#   max_density           reference 1030 of 3010 (maxDensity = the median density, 2048 dense points)
#   point_to_point        reference 1966 of 4096
#   reading               reading 946 of 2031
#   both                  reference 1966 of 4096, reading 922 of 2018
def cases(md="26.893463"):
    return {
        "sampling": chain(reference=SSN + shadow()),
        "surface_normal": chain(reference=SN + PAIR_REF + shadow()),
        "max_density": chain(reference=SN_DENS + max_density(md) + shadow() + PAIR_REF),
        "point_to_point": chain(reference=SN + shadow(), minimizer="PointToPointErrorMinimizer"),
        "reading": chain(reading=RS + SN_RD + PAIR_RD + shadow(), reference=SSN + PAIR_REF, outliers=TRIM + SNO),
        "both": chain(reading=RS + SN_RD + shadow() + PAIR_RD, reference=SN + shadow() + PAIR_REF, outliers=TRIM + SNO),
    }


def stream_position():
    """A fingerprint of where the library's draw stream stands: which of its next 64 draws are below 0.5 (consumes them)"""
    from laser_slam_amd import icp
    return tuple(int(i) for i in icp.random_sampling(64, 0.5, seed=-1))


def trace_bytes(h):
    out = b""
    for t in h.trace():
        out += np.ascontiguousarray(t["T_iter"]).tobytes() + np.float32(t["limit"]).tobytes() + np.int64(t["n_used"]).tobytes()
        out += np.ascontiguousarray(t["A"]).tobytes() + np.ascontiguousarray(t["b"]).tobytes() + np.ascontiguousarray(t["x"]).tobytes()
    return out


def result(T, st, h):
    """what the two routes must agree on"""
    return (np.ascontiguousarray(T).tobytes(), int(st.iterations), int(st.converged), np.float32(st.final_limit).tobytes(),
            int(st.final_n_used), trace_bytes(h), int(h.info().n_reference))


def route_a(doc, rd, ref, T_init, seed=SEED):
    """the loaded document through the Python facade -> (result, stream position)"""
    from laser_slam_amd import icp
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(doc))
    o.chain.seed = seed
    T = o.compute(rd, ref, T_init)
    r = result(T, o.last_stats, o.handle)
    pos = stream_position()
    o.handle.close()
    return r, pos


def route_b(doc, rd, ref, T_init, seed=SEED):
    """the same compute by hand -> (result, stream position, {side: (points handed to the module, points it kept)})"""
    from laser_slam_amd import icp, _lib
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(doc))
    ch = o.chain
    rd_eps, ref_eps = ch.shadow
    nc = ch.normals
    counts = {}
    with icp.IcpHandle() as hf:
        icp.random_sampling(0, 0.5, seed=seed)                         # the chain seed
        if ch.surface_normal_knn > 0:
            rf, rn = hf.filter_reference(ref, ch.surface_normal_knn, ch.surface_normal_ratio, seed=-1)
        elif ch.max_density is not None:
            rf, rn, _n_dense = hf.filter_reference_max_density(ref, ch.reference_normal_knn, ch.max_density, seed=-1)
        else:
            rf, rn = np.ascontiguousarray(ref, np.float32), hf.filter_reference_normals(ref, ch.reference_normal_knn)
        rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
        if ref_eps is not None:
            n_in = len(rf)
            rf, rn = icp.shadow(rf, rn, ref_eps)                       # the HOST twin
            counts["reference"] = (n_in, len(rf))
        if nc is not None and nc.reference_orient:
            rn = icp.orient_normals(rf, rn, nc.reference_sensor, nc.reference_orient == 1)
        rdk = np.ascontiguousarray(hf.filter_reading(rd, ch.reading_sampling_prob, seed=-1))
        rdn = None
        if nc is not None and nc.reading_sn_knn > 0:
            rdn = hf.reading_normals(rdk, nc.reading_sn_knn, nc.reading_orient, nc.reading_sensor)
            if rd_eps is not None:
                n_in = len(rdk)
                rdk, rdn = icp.shadow(rdk, rdn, rd_eps)                # the HOST twin
                counts["reading"] = (n_in, len(rdk))
    pos = stream_position()
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.trim_ratio, cfg.max_iterations = ch.trim_ratio, ch.max_iterations
    cfg.min_diff_rot, cfg.min_diff_trans, cfg.smooth_length = ch.min_diff_rot, ch.min_diff_trans, ch.smooth_length
    angle = nc is not None and nc.max_angle >= 0
    normals = dict(max_angle=nc.max_angle, reading_normals_given=1) if angle else None
    p2p = ch.error_minimizer == "PointToPointErrorMinimizer"
    with icp.IcpHandle(cfg, 0, ch.error_minimizer, ch.matcher_knn, ch.matcher_max_dist, ch.outlier_max_dist, ch.outlier_min_dist,
                       ch.outlier_median_factor, normals=normals) as h:
        h.set_reference(rf, None if p2p else rn)
        T, st = h.align_normals(rdk, rdn, T_init) if angle else h.align(rdk, T_init)
        return result(T, st, h), pos, counts


def digest(r, pos):
    return hashlib.sha256(b"".join(x if isinstance(x, bytes) else repr(x).encode() for x in r) + repr(pos).encode()).hexdigest()


SIDE_CASES = ("sampling", "surface_normal", "point_to_point")   # the chains whose reading runs on the side stream


def main():
    """Both routes of the side-stream chains in this process (started with LSGPU_NO_SIDE_STREAM=1: switches are read once)
    -> one JSON line"""
    from laser_slam_amd import synth
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    out = {}
    for name in SIDE_CASES:
        doc = cases()[name]
        a, pos_a = route_a(doc, rd, ref, T_init)
        b, pos_b, _counts = route_b(doc, rd, ref, T_init)
        out[name] = {"a": digest(a, pos_a), "b": digest(b, pos_b)}
    print("SHADOW_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
