"""What tests/test_covariance_sampling.py shares between its cases, and (run as a program) the worker of its side-stream case.

The identity under test: ICP.compute on a loaded document with CovarianceSamplingDataPointsFilter (route a) equals the same
compute assembled by hand (route b) -- the section's other modules by the library's kernel-level entries, the module itself
by lsgpu_icp_filter_cov_sampling, then set_reference + align / align_normals on a handle that has never heard of the module:
T_out, the result fields of the stats, the trace records and the position of the library's draw stream, bit for bit.  The
document builders and the result's fingerprint are those of tests/shadow_cases.py."""
import ctypes as C
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

from shadow_cases import (PAIR_RD, PAIR_REF, RS, SN, SN_DENS, SN_RD, SNO, SSN, TRIM, chain, digest, max_density, result,  # noqa: F401
                          shadow, stream_position, trace_bytes)

SEED = 4
F = np.float32


def cov_sampling(nb=None, tq=None):
    y = "  - CovarianceSamplingDataPointsFilter"
    if nb is None and tq is None:
        return y + "\n"
    y += ":\n"
    if nb is not None:
        y += "      nbSample: %s\n" % nb
    if tq is not None:
        y += "      torqueNorm: %s\n" % tq
    return y


MAX_DIST_10 = "  - MaxDistDataPointsFilter:\n      maxDist: 10\n"   # keeps 3226 of the pair's 4096 reference points

P2P = "PointToPointErrorMinimizer"


# The cases of the compute test on the 4 k-point pair (4096 reference points, 4080 reading points), seed 4; what the module is
# handed is asserted to be more than nbSample in the test.  The chains of several thinning stages, counted with the host
# twins (every stage is asserted to drop something in the test):
#   sn_shadow, sn_shadow_point_to_point        Shadow keeps 2130 of 4096, the module 1000 of them
#   sn_max_density_shadow                      MaxDensity keeps 3010 of 4096 (maxDensity = the median density), Shadow 1980 of
#                                              them, the module 900 of them
#   sn_max_density_point_to_point              MaxDensity keeps 3010 of 4096; no module, and nobody reads the normals
def cases(md="26.893463"):
    return {
        "sn_shadow": chain(reference=SN + shadow() + cov_sampling(1000, 1) + PAIR_REF),
        "sn_max_density_shadow": chain(reference=SN_DENS + max_density(md) + shadow() + cov_sampling(900, 1) + PAIR_REF),
        "sn_max_density_point_to_point": chain(reference=SN_DENS + max_density(md), minimizer=P2P),
        "sn_shadow_point_to_point": chain(reference=SN + shadow() + cov_sampling(1000, 2), minimizer=P2P),
        "sampling": chain(reference=SSN + cov_sampling(600, 1)),
        "surface_normal": chain(reference=SN + PAIR_REF + cov_sampling(1500, 2)),
        "max_density": chain(reference=SN_DENS + max_density(md) + cov_sampling(1000, 1) + PAIR_REF),
        "shadow": chain(reference=SSN + shadow() + cov_sampling(500, 0)),
        "point_to_point": chain(reference=SN + cov_sampling(1500, 1), minimizer=P2P),
        "reading": chain(reading=RS + SN_RD + PAIR_RD + cov_sampling(800, 1), reference=SSN + PAIR_REF, outliers=TRIM + SNO),
        "both": chain(reading=RS + SN_RD + cov_sampling(800, 2) + PAIR_RD, reference=SN + cov_sampling(1500, 0) + PAIR_REF,
                      outliers=TRIM + SNO),
    }


def fallback_cases(nb):
    """SurfaceNormalDataPointsFilter with the module alone behind it and an nbSample that reaches what the module is handed: the
    section passes unchanged.  -> {name: (the document, the same document without the module)}; "cut": a cut module in front
    leaves 3226 points, which nbSample reaches although it is below 4096"""
    return {
        "plain": (chain(reference=SN + cov_sampling(nb, 1) + PAIR_REF), chain(reference=SN + PAIR_REF)),
        "point_to_point": (chain(reference=SN + cov_sampling(nb, 1), minimizer=P2P), chain(reference=SN, minimizer=P2P)),
        "cut": (chain(reference=MAX_DIST_10 + SN + cov_sampling(nb, 1) + PAIR_REF), chain(reference=MAX_DIST_10 + SN + PAIR_REF)),
    }


def corridor(n_wall=2000, n_floor=2000, n_end=80, seed=5):
    """A corridor: a floor (z = 0), two long parallel walls (x in [0, 40], y = +-1.5, z in [0, 2.5]) and an end wall at x = 40
    that holds n_end of the points; the normals are the surfaces' own (exact), the points jittered by 5 mm.  Without the floor
    no normal has a z component, C has an exactly zero eigenvalue, t[0] stays 0 and the walk never leaves list 0.
    -> (xyz1, normals, mask of the end-wall points), shuffled"""
    rng = np.random.default_rng(seed)
    parts, nrm, end = [], [], []
    for y in (-1.5, 1.5):
        p = np.stack([rng.uniform(0, 40, n_wall), np.full(n_wall, y), rng.uniform(0, 2.5, n_wall)], axis=1)
        parts.append(p); nrm.append(np.tile([0.0, -np.sign(y), 0.0], (n_wall, 1))); end.append(np.zeros(n_wall, bool))
    p = np.stack([rng.uniform(0, 40, n_floor), rng.uniform(-1.5, 1.5, n_floor), np.zeros(n_floor)], axis=1)
    parts.append(p); nrm.append(np.tile([0.0, 0.0, 1.0], (n_floor, 1))); end.append(np.zeros(n_floor, bool))
    p = np.stack([np.full(n_end, 40.0), rng.uniform(-1.5, 1.5, n_end), rng.uniform(0, 2.5, n_end)], axis=1)
    parts.append(p); nrm.append(np.tile([-1.0, 0.0, 0.0], (n_end, 1))); end.append(np.ones(n_end, bool))
    p, v, e = np.concatenate(parts), np.concatenate(nrm), np.concatenate(end)
    p = p + rng.normal(scale=0.005, size=p.shape)
    order = rng.permutation(len(p))
    xyz1 = np.ones((len(p), 4), F)
    xyz1[:, :3] = p[order]
    return xyz1, np.ascontiguousarray(v[order], F), e[order]


def random_cloud(n, seed=0):
    """n points of an anisotropic blob off the origin, unit-ish normals, the 4th component anything"""
    rng = np.random.default_rng(seed * 7919 + n)
    p = np.ones((n, 4), F)
    p[:, :3] = rng.normal(size=(n, 3)) * [10, 3, 1] + [5, 2, 1]
    p[:, 3] = rng.uniform(0, 2, n)
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.9, 1.1, (n, 1))).astype(F)
    return p, v


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
    """the same compute by hand -> (result, stream position, {side: (points handed to the module, points it kept)}; the other
    thinning stages of the reference as "reference MaxDensity" / "reference Shadow")"""
    from laser_slam_amd import icp, _lib
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(doc))
    ch = o.chain
    cs_rd, cs_ref = ch.cov_sampling if ch.cov_sampling is not None else (None, None)
    sh_rd, sh_ref = ch.shadow if ch.shadow is not None else (None, None)
    nc = ch.normals
    counts = {}
    with icp.IcpHandle() as hf:
        icp.random_sampling(0, 0.5, seed=seed)                         # the chain seed
        if ch.surface_normal_knn > 0:
            rf, rn = hf.filter_reference(ref, ch.surface_normal_knn, ch.surface_normal_ratio, seed=-1)
        elif ch.max_density is not None:
            rf, rn, _n_dense = hf.filter_reference_max_density(ref, ch.reference_normal_knn, ch.max_density, seed=-1)
            counts["reference MaxDensity"] = (len(ref), len(rf))
        else:
            rf, rn = np.ascontiguousarray(ref, np.float32), hf.filter_reference_normals(ref, ch.reference_normal_knn)
        rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
        if sh_ref is not None:
            n_in = len(rf)
            rf, rn = hf.filter_shadow(rf, rn, sh_ref)
            rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
            counts["reference Shadow"] = (n_in, len(rf))
        if cs_ref is not None:
            n_in = len(rf)
            rf, rn, _ids = hf.filter_cov_sampling(rf, rn, cs_ref[0], cs_ref[1])
            rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
            counts["reference"] = (n_in, len(rf))
        if nc is not None and nc.reference_orient:
            rn = icp.orient_normals(rf, rn, nc.reference_sensor, nc.reference_orient == 1)
        rdk = np.ascontiguousarray(hf.filter_reading(rd, ch.reading_sampling_prob, seed=-1))
        rdn = None
        if nc is not None and nc.reading_sn_knn > 0:
            rdn = hf.reading_normals(rdk, nc.reading_sn_knn, nc.reading_orient, nc.reading_sensor)
            if sh_rd is not None:
                rdk, rdn = hf.filter_shadow(rdk, rdn, sh_rd)
            if cs_rd is not None:
                n_in = len(rdk)
                rdk, rdn, _ids = hf.filter_cov_sampling(np.ascontiguousarray(rdk), np.ascontiguousarray(rdn), cs_rd[0], cs_rd[1])
                rdk, rdn = np.ascontiguousarray(rdk), np.ascontiguousarray(rdn)
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


SIDE_CASES = ("sampling", "sn_shadow")   # chains whose reading runs on the side stream


def main():
    """Both routes of the side-stream chain in this process (started with LSGPU_NO_SIDE_STREAM=1: switches are read once) -> one
    JSON line"""
    from laser_slam_amd import synth
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    out = {}
    for name in SIDE_CASES:
        doc = cases()[name]
        a, pos_a = route_a(doc, rd, ref, T_init)
        b, pos_b, _counts = route_b(doc, rd, ref, T_init)
        out[name] = {"a": digest(a, pos_a), "b": digest(b, pos_b)}
    print("COV_SAMPLING_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
