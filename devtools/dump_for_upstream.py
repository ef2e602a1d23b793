#!/usr/bin/env python3
"""Everything somebody WITH libpointmatcher needs to diff the restatement this library was written against
(oracle/icp_oracle.c; "parity unpinned": SURVEY.md 8c) against upstream -- CPU only, no GPU, deterministic.

For a synthetic HDL-64E pair (default: the 4 k-point pair of the parity tests, `--n-az 1024` = the 64 k pair) it writes

  reading.vtk / .csv, reference.vtk / .csv   the RAW clouds `icp_.compute(reading, reference, T_init)` is handed
                                             (laser_slam/src/laser_track.cpp:496), as DataPoints::load reads them
  icp.yaml                                   the module chain (tests/golden/icp_chain*.yaml, loadable by
                                             PointMatcher::ICP::loadFromYaml; checked here with this repo's own loader)
  T_init.txt                                 4 x 4, row major, "%.9g"
  reference_filtered.csv                     what SamplingSurfaceNormalDataPointsFilter leaves (x,y,z,nx,ny,nz): choices 1, 2, 8, 10, 11
                                             (a chain with SurfaceNormalDataPointsFilter keepDensities 1 + MaxDensityDataPointsFilter:
                                             what those leave, and reference_densities.csv with every reference point's density:
                                             choices 36-40; such a chain's draws, the reading's included, come from the
                                             library's own stream, so --submap, whose input filters draw from the oracle's,
                                             refuses it; a chain with ShadowDataPointsFilter in the reference section:
                                             what is left behind that module too -- the library's host twin, no draw:
                                             choices 41-44; the module on the reading is refused, the oracle's loop reads no
                                             reading normals; a chain with CovarianceSamplingDataPointsFilter in the reference
                                             section: what that module picks, in pick order -- the library's host twin, no
                                             draw: choices 55-62; on the reading it is refused for the same reason)
  reading_filtered.csv                       what RandomSamplingDataPointsFilter leaves: choice 8 (the draws continue the
                                             reference filter's; the process starts at srand(1) like an unseeded one)
  input_filtered.csv                         reading.csv through tests/golden/input_filters.yaml (srand(1) again): choice 9
  input_filters.yaml                         only with --voxel-grid VX,VY,VZ[,useCentroid]: the golden input chain with a
                                             VoxelGridDataPointsFilter appended -- the chain input_filtered.csv (and, with
                                             --submap, scan*_input_filtered.csv) then went through: choices 30-34;
                                             likewise with --octree-grid MAX_SIZE,MAX_POINT[,SAMPLING_METHOD]: an
                                             OctreeGridDataPointsFilter appended (behind the voxel grid if both are asked
                                             for): choices 49-54 (samplingMethod 1, RandomPts, is refused: its draws would
                                             come from the library's stream, the chain's other modules draw from the oracle's)
  oracle_trace.csv                           per iteration: iter, limit (squared metres), n_used, T_iter (16, column major)
  oracle_result.txt                          rc, iterations, converged, final T (4 x 4 row major)
  README.txt                                 what is what, and which file / column each restatement choice would change

With --submap the dump has the REAL call shape of LaserTrack::localScanToSubMap (laser_slam/src/laser_track.cpp:466-519)
instead of a bare pair: four scans along a trajectory go through the input filter chain (input_filters_.apply, :146), the
sub-map is assembled from the three older ones in the frame of the newest of them (RigidTransformation::compute with the
float relative pose + concatenate, :474-486), the guess is T_a^-1 T_b of the odometry poses (:489-491):
  scan{0..3}.vtk / .csv                      the raw scans           scan{0..3}_input_filtered.csv   after the input chain (one
                                                                     draw stream over the four scans, srand(1) before the first)
  poses.txt                                  the four odometry poses T_w_scan (4 x 4 row major each)
  T_rel{1,2}.txt                             the float relative poses the two older scans are moved by
  reading.csv / reference.csv / T_init.txt   what icp_.compute is handed: scan 3 filtered, the assembled sub-map, the guess
  reference_filtered.csv, reading_filtered.csv, oracle_trace.csv, oracle_result.txt   as above (the ICP's own draw stream
                                             continues the input filters': one process, one rand())

The files regenerate byte for byte (tests/test_oracle.py::test_upstream_dump_regenerates).  INTEGRATION.md has the
C++ program that replays them on a real PointMatcher<float>::ICP and prints a trace in the same format.
usage: dump_for_upstream.py OUT_DIR [--n-az 64] [--chain tests/golden/icp_chain_tight.yaml] [--submap] [--voxel-grid 0.5,0.5,0.5]
                            [--octree-grid 0.5,7,3]
"""
import argparse
import ctypes as C
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from laser_slam_amd import cloud_io, synth  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

CHOICES = """Restatement choices of oracle/icp_oracle.h and where a different upstream behaviour shows:
 1 box rank test (FullPivHouseholderQR, eps * 3)      reference_filtered.csv: number of rows (thin boxes kept / dropped)
 2 box split (stable sort, split at the median)      reference_filtered.csv: normals of boxes with tied coordinates; for ratio < 1 WHICH rows
 3 kd-tree ties (any nearest point)                  nothing: oracle_trace.csv is the same for every valid tie order
 4 TrimmedDist: index floor(n * ratio), d2 <= limit  oracle_trace.csv: columns limit and n_used
 5 reference mean in double, rounded to float        oracle_trace.csv: last digits of T_iter (1e-6 level)
 6 minimiser: float J, LLT solve in float            oracle_trace.csv: T_iter from the first iteration on
 7 differential checker: 2 atan2(|vec|, |w|)         oracle_trace.csv: number of rows (the iteration it stops at)
 8 rand(): glibc sequence, draw < prob keeps         reading_filtered.csv (and reference_filtered.csv for ratio < 1): WHICH rows
 9 MaxDist signed on one axis, MinDist absolute      input_filtered.csv: rows
10 kept points in ascending ORIGINAL index             reference_filtered.csv: row order (upstream sorts indicesToKeep before it compacts)
11 box eigenvectors: Jacobi in double on the float C   reference_filtered.csv: last digits of nx, ny, nz (upstream: EigenSolver in float)
"""
VOXEL_CHOICES = """30 VoxelGrid: float bounds, numDiv = (uint)((1 + maxB) - minB)   input_filtered.csv: number of rows
31 VoxelGrid: cell indices clamped to numDiv - 1                 input_filtered.csv: rows at the cloud's upper faces
32 VoxelGrid: centroid = first point + the others in input order, / count   input_filtered.csv: last digits of x, y, z
33 VoxelGrid: output in the order of the voxels' first points    input_filtered.csv: row order
34 VoxelGrid: the pad row and descriptors are the first point's  input_filtered.csv: nothing (pad is 1)
"""
OCTREE_CHOICES = """49 OctreeGrid: root centre min + ext 0.5, radius = the largest extent 0.5; octant by x > cx, y > cy, z > cz   input_filtered.csv: WHICH rows / number of rows
50 OctreeGrid: a leaf at 2 radius <= maxSizeByNode, at <= maxPointByNode points, or at depth 21 (the cap is a DEVIATION)   input_filtered.csv: number of rows
51 OctreeGrid: output point k comes from the k-th non-empty leaf, depth first, octants 0..7             input_filtered.csv: row order
52 OctreeGrid: FirstPts = smallest input index; RandomPts = point (uint)((count - 1) draw), one draw per leaf   input_filtered.csv: WHICH rows
53 OctreeGrid: centroid = first point + the others in input order, / count; medoid = nearest to it, the earliest of a tie   input_filtered.csv: last digits / WHICH rows
54 OctreeGrid: the pad row and descriptors are the chosen point's (Centroid: the first point's pad)   input_filtered.csv: nothing (pad is 1)
"""
DENSITY_CHOICES = """36 density: knn / ((4/3) pi r^3), r = the largest distance from the neighbourhood's mean, float   reference_densities.csv: last digits
37 density of knn identical points: +inf (dropped by MaxDensity)   reference_densities.csv: inf rows; reference_filtered.csv: rows
38 MaxDensity: one draw per point with density > maxDensity, kept iff draw < maxDensity / density   reference_filtered.csv: WHICH rows
39 MaxDensity: the densest points' acceptance times (1 - nbSaturated / n) as an integer division   reference_filtered.csv: rows of the densest points
40 the reading's draws continue behind the dense points' draws   reading_filtered.csv: WHICH rows
"""
SHADOW_CHOICES = """41 Shadow: value = |n/|n| . p/|p||, float, three divisions per vector, sums left to right   reference_filtered.csv: WHICH rows (points near eps)
42 Shadow: kept iff value > eps (a tie is dropped)                  reference_filtered.csv: rows whose value equals eps
43 Shadow: a zero normal, a point at the origin, a NaN: dropped    reference_filtered.csv: those rows
44 Shadow: p is the point as given to the section, the sensor at the frame's origin   reference_filtered.csv: WHICH rows
"""
COV_SAMPLING_CHOICES = """55 CovarianceSampling: c = (float)(sum p / n) in double, v = (invL (p - c) x n, n) in float      reference_filtered.csv: WHICH rows
56 CovarianceSampling: Lnorm 1 / mean |p - c| / half the largest extent (torqueNorm 0 / 1 / 2)     reference_filtered.csv: WHICH rows
57 CovarianceSampling: C = sum v v^T in double; cyclic Jacobi in double, vectors rounded to float      reference_filtered.csv: WHICH rows (near-tied magnitudes)
58 CovarianceSampling: eigen-directions in ASCENDING order of the eigenvalue (upstream: unspecified)   reference_filtered.csv: WHICH rows and their order
59 CovarianceSampling: lists by decreasing |v . X_k|, ties by ascending index (stable sort)          reference_filtered.csv: rows with tied magnitudes
60 CovarianceSampling: the walk takes the FIRST index of the smallest t; t_j += mag_j^2 in float      reference_filtered.csv: WHICH rows and their order
61 CovarianceSampling: output in pick order, every component of point and normal                     reference_filtered.csv: row order
62 CovarianceSampling: nbSample >= n passes the cloud unchanged; Lnorm 0 / a value not finite is an error   reference_filtered.csv: all rows / no dump
"""
MOTION_CHOICES = """45 force2D / force4DOF: rows and columns {2,3,4} / {2,3,4,5} of the 6x6 system, float LLT   T of every iteration
46 force2D: b with the planar residual n.x dx + n.y dy, normals not renormalised; matching and filters stay 3-D   T of every iteration
47 constrained dT: third row and column exactly 0 0 1, sine / cosine of |yaw| in double   T of every iteration (last bits)
48 BoundTransformationChecker: against the loop's first T_iter (identity, reference-mean frame), compared with >   WHETHER compute throws
(oracle_trace.csv / oracle_result.txt are the oracle's FREE 6-DOF loop without the bound -- the oracle restates neither module;
 the library's own records of this chain: ICP.compute, then IcpHandle.trace())
"""


def g(v) -> str:
    return "%.9g" % float(v)


def parse_chain(path):
    """The chain file through this repo's own loader (laser_slam_amd.icp.ICP.load_from_yaml): the values the oracle runs."""
    from laser_slam_amd import icp
    m = icp.ICP()
    m.load_from_yaml(path)
    return m.chain


def voxel_grid_yaml(vsize=(1.0, 1.0, 1.0), use_centroid=1, average_existing_descriptors=1) -> str:
    """The module as one item of a libpointmatcher DataPointsFilters file ("%.9g": the float comes back bit for bit)."""
    return ("- VoxelGridDataPointsFilter:\n    vSizeX: %s\n    vSizeY: %s\n    vSizeZ: %s\n    useCentroid: %d\n"
            "    averageExistingDescriptors: %d\n" % (g(np.float32(vsize[0])), g(np.float32(vsize[1])), g(np.float32(vsize[2])),
                                                       int(use_centroid), int(average_existing_descriptors)))


def octree_grid_yaml(max_size_by_node=0.0, max_point_by_node=1, sampling_method=0, build_parallel=1) -> str:
    """OctreeGridDataPointsFilter as one item of a libpointmatcher DataPointsFilters file."""
    return ("- OctreeGridDataPointsFilter:\n    buildParallel: %d\n    maxPointByNode: %d\n    maxSizeByNode: %s\n    samplingMethod: %d\n"
            % (int(build_parallel), int(max_point_by_node), g(np.float32(max_size_by_node)), int(sampling_method)))


def input_filter_chain(path, text=None):
    """tests/golden/input_filters.yaml (or the text of such a file) -> oracle PointFilter array.  VoxelGridDataPointsFilter
    (type 7) and OctreeGridDataPointsFilter (type 8) are not in the oracle: run_input_filters hands them to the library's
    host twins."""
    import yaml
    doc = yaml.safe_load(open(path).read() if text is None else text) or []
    arr = (O.PointFilter * len(doc))()
    for a, item in zip(arr, doc):
        (name, p), = item.items() if isinstance(item, dict) else ((item, {}),)
        p = p or {}
        a.state = 0.0
        if name == "BoundingBoxDataPointsFilter":
            a.type, a.flag = 3, int(p.get("removeInside", 1))
            for i, k in enumerate(("xMin", "xMax", "yMin", "yMax", "zMin", "zMax")):
                a.v[i] = float(p.get(k, -1.0 if i % 2 == 0 else 1.0))
        elif name == "MaxDistDataPointsFilter":
            a.type, a.dim = 1, int(p.get("dim", -1)); a.v[0] = float(p.get("maxDist", 1.0))
        elif name == "MinDistDataPointsFilter":
            a.type, a.dim = 2, int(p.get("dim", -1)); a.v[0] = float(p.get("minDist", 1.0))
        elif name == "FixStepSamplingDataPointsFilter":
            a.type = 4; a.v[0] = float(p.get("startStep", 10)); a.v[1] = float(p.get("endStep", 10)); a.v[2] = float(p.get("stepMult", 1))
        elif name == "RandomSamplingDataPointsFilter":
            a.type = 5; a.v[0] = float(p.get("prob", 0.75))
        elif name == "RemoveNaNDataPointsFilter":
            a.type = 6
        elif name == "VoxelGridDataPointsFilter":
            a.type, a.flag, a.dim = 7, int(p.get("useCentroid", 1)), int(p.get("averageExistingDescriptors", 1))
            for i, k in enumerate(("vSizeX", "vSizeY", "vSizeZ")):
                a.v[i] = float(p.get(k, 1.0))
        elif name == "OctreeGridDataPointsFilter":
            a.type, a.dim, a.flag = 8, int(p.get("samplingMethod", 0)), int(p.get("buildParallel", 1))
            a.v[0] = float(p.get("maxSizeByNode", 0.0)); a.v[1] = float(p.get("maxPointByNode", 1))
        else:
            raise SystemExit("input filter %s is not in the restatement" % name)
    return arr


def run_input_filters(flt, cloud, seed):
    """The chain on one cloud: the oracle for every run of its own modules (one draw stream, `seed` before the first), the
    host twins of the library (lsgpu_filter_voxel_grid_points, lsgpu_filter_octree_grid_points, no GPU) for
    VoxelGridDataPointsFilter and OctreeGridDataPointsFilter, which draw nothing (RandomPts is refused when the chain is made).
    None if a module is handed an empty cloud."""
    from laser_slam_amd import icp
    i, n = 0, len(flt)
    while i < n and cloud is not None:
        if cloud.shape[0] == 0:
            return None
        if flt[i].type == 7:
            cloud = icp.voxel_grid_points(cloud, [flt[i].v[k] for k in range(3)], flt[i].flag)
            i += 1
            continue
        if flt[i].type == 8:
            cloud = icp.octree_grid_points(cloud, flt[i].v[0], int(flt[i].v[1]), flt[i].dim)
            i += 1
            continue
        j = i
        while j < n and flt[j].type not in (7, 8):
            j += 1
        part = (O.PointFilter * (j - i)).from_address(C.addressof(flt) + i * C.sizeof(O.PointFilter))   # (FixStep's state stays in flt)
        cloud = O.apply_point_filters(part, cloud, seed=seed)
        seed, i = -1, j
    return cloud


def write_mat(path, T):
    with open(path, "w") as f:
        for r in range(4):
            f.write(" ".join(g(T[r, c]) for c in range(4)) + "\n")


def input_chain_for_dump(out_dir, voxel_grid, octree_grid=None):
    """The golden input chain; with `voxel_grid` (vSizeX, vSizeY, vSizeZ[, useCentroid]) and / or `octree_grid` (maxSizeByNode,
    maxPointByNode[, samplingMethod]) the modules are appended and the chain's text written to OUT_DIR/input_filters.yaml."""
    path = os.path.join(ROOT, "tests", "golden", "input_filters.yaml")
    if not voxel_grid and not octree_grid:
        return input_filter_chain(path)
    text = open(path).read().rstrip("\n") + "\n"
    if voxel_grid:
        text += voxel_grid_yaml(voxel_grid[:3], int(voxel_grid[3]) if len(voxel_grid) > 3 else 1, 0)
    if octree_grid:
        method = int(octree_grid[2]) if len(octree_grid) > 2 else 0
        if method == 1:
            # the chain's other modules draw from the oracle's rand(), the host twin from the library's own stream: the two
            # cannot continue one another (the rule of --submap with MaxDensityDataPointsFilter)
            raise SystemExit("--octree-grid with samplingMethod 1 (RandomPts) is not supported: its draws (the library's stream) and "
                             "the other input filters' (the oracle's rand()) would not be one sequence")
        text += octree_grid_yaml(octree_grid[0], int(octree_grid[1]), method)
    with open(os.path.join(out_dir, "input_filters.yaml"), "w") as f:
        f.write(text)
    return input_filter_chain(None, text)


def submap_inputs(out_dir, n_az, voxel_grid=None, octree_grid=None):
    """laser_track.cpp:146, 466-496 on four synthetic scans: input filters, sub-map of three in the frame of scan 2, the
    odometry guess.  Returns (reading, reference, T_init 4x4 float64, seed for the ICP's first draw)."""
    scene = synth.Scene(1234)
    truth = [synth.se3(0.8 * i, 0.05 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(2.0 * i)) for i in range(4)]
    odom = [T @ synth.se3(0.1, -0.05, 0.0, yaw=np.deg2rad(0.5)) for T in truth]     # (the drive of bench.py's value_track)
    flt = input_chain_for_dump(out_dir, voxel_grid, octree_grid)
    filtered = []
    with open(os.path.join(out_dir, "poses.txt"), "w") as f:
        for i in range(4):
            raw = synth.hdl64_scan(scene, truth[i], n_az, 10 + i)
            cloud_io.save_vtk(os.path.join(out_dir, "scan%d.vtk" % i), raw)
            cloud_io.save_csv(os.path.join(out_dir, "scan%d.csv" % i), raw)
            kept = run_input_filters(flt, raw, 1 if i == 0 else -1)                # one process, one rand() stream
            kept = kept if kept is not None else raw[:0]
            cloud_io.save_csv(os.path.join(out_dir, "scan%d_input_filtered.csv" % i), kept)
            filtered.append(kept)
            for r in range(4):
                f.write(" ".join(g(odom[i][r, c]) for c in range(4)) + "\n")
    a = 2                                                                           # the sub-map's frame: the newest of its scans
    parts = [filtered[a]]
    for n, k in enumerate((1, 0), start=1):
        Trel = (np.linalg.inv(odom[a]) @ odom[k]).astype(np.float32)               # TransformationParameters are float
        write_mat(os.path.join(out_dir, "T_rel%d.txt" % n), Trel)
        parts.append(O.transform_points(synth.colmajor(Trel), filtered[k]))        # RigidTransformation::compute
    return filtered[3], np.ascontiguousarray(np.concatenate(parts, 0)), np.linalg.inv(odom[a]) @ odom[3], -1


def dump(out_dir, n_az, chain_path, submap=False, voxel_grid=None, octree_grid=None):
    os.makedirs(out_dir, exist_ok=True)
    ch = parse_chain(chain_path)
    if submap and ch.max_density is not None:
        # the input filters of the four scans draw from the oracle's rand(), MaxDensityDataPointsFilter's host twin from the
        # library's own stream: the two cannot continue one another, and a dump with two streams would not be one process's
        raise SystemExit("--submap with MaxDensityDataPointsFilter in the chain is not supported: the input filters' draws (the "
                         "oracle's rand()) and the reference section's (the library's stream) would not be one sequence")
    if ch.shadow is not None and ch.shadow[0] is not None:
        # the reading's module stands behind the reading's normals, which only SurfaceNormalOutlierFilter reads: not in the oracle's loop
        raise SystemExit("ShadowDataPointsFilter in readingDataPointsFilters is not supported: the oracle's loop runs no "
                         "SurfaceNormalOutlierFilter and reads no reading normals")
    if ch.cov_sampling is not None and ch.cov_sampling[0] is not None:
        raise SystemExit("CovarianceSamplingDataPointsFilter in readingDataPointsFilters is not supported: the oracle's loop runs no "
                         "SurfaceNormalOutlierFilter and reads no reading normals")
    shutil.copyfile(chain_path, os.path.join(out_dir, "icp.yaml"))
    if submap:
        rd, ref, T_init, icp_seed = submap_inputs(out_dir, n_az, voxel_grid, octree_grid)
    else:
        ref, rd, T_true, T_init = synth.scan_pair(n_az)
        icp_seed = 1
        cloud_io.save_vtk(os.path.join(out_dir, "reading.vtk"), rd)
        cloud_io.save_vtk(os.path.join(out_dir, "reference.vtk"), ref)
    cloud_io.save_csv(os.path.join(out_dir, "reading.csv"), rd)
    cloud_io.save_csv(os.path.join(out_dir, "reference.csv"), ref)
    T16 = synth.colmajor(T_init)
    write_mat(os.path.join(out_dir, "T_init.txt"), T16.reshape(4, 4).T)
    # ICP::compute, steps 1 and 4 with ONE draw stream that starts where an unseeded process starts (srand(1)) -- or, in the
    # sub-map dump, where the input filters of the four scans left it
    if ch.max_density is not None:
        # SurfaceNormalDataPointsFilter keepDensities 1 + MaxDensityDataPointsFilter [+ the orientation pair]: not in the oracle,
        # the library's host twins (no GPU): choices 36-40; reference_densities.csv has the density of every reference point
        from laser_slam_amd import icp
        # The twins draw from the LIBRARY's stream (csrc/lsgpu_rand.h: glibc's sequence, never libc's state), so the reading's
        # mask is taken from that stream as well: draws n_dense + 1 .. n_dense + nq of srand(icp_seed), choice 40
        rf, rn, _n_dense, dens = icp.max_density(ref, ch.reference_normal_knn, ch.max_density, icp_seed)
        if ch.normals is not None and ch.normals.reference_orient:
            rn = icp.orient_normals(rf, rn, ch.normals.reference_sensor, ch.normals.reference_orient == 1)
        np.savetxt(os.path.join(out_dir, "reference_densities.csv"), dens, fmt="%.9g")
        rdf = rd[icp.random_sampling(rd.shape[0], ch.reading_sampling_prob, -1)] if ch.reading_sampling_prob >= 0 else rd
    else:
        rf, rn = O.sampling_surface_normal(ref, ch.surface_normal_knn, ch.surface_normal_ratio, icp_seed)
        rdf = rd[O.random_sampling(rd.shape[0], ch.reading_sampling_prob, -1)] if ch.reading_sampling_prob >= 0 else rd
    if ch.shadow is not None:
        # ShadowDataPointsFilter behind the reference's normals (in front of or behind the orientation pair: |dot| is the same):
        # not in the oracle, the library's host twin; no draw: choices 41-44
        from laser_slam_amd import icp
        rf, rn = icp.shadow(rf, rn, ch.shadow[1])
    if ch.cov_sampling is not None:
        # CovarianceSamplingDataPointsFilter, the section's last thinning step (in front of or behind the orientation pair: the
        # module does not read the normals' signs): not in the oracle, the library's host twin; no draw: choices 55-62
        from laser_slam_amd import icp
        rf, rn, _ids = icp.cov_sampling(rf, rn, ch.cov_sampling[1][0], ch.cov_sampling[1][1])
    cloud_io.save_csv(os.path.join(out_dir, "reference_filtered.csv"), rf, rn)
    cloud_io.save_csv(os.path.join(out_dir, "reading_filtered.csv"), rdf)
    if not submap:
        flt = input_chain_for_dump(out_dir, voxel_grid, octree_grid)
        kept = run_input_filters(flt, rd, 1)
        cloud_io.save_csv(os.path.join(out_dir, "input_filtered.csv"), kept if kept is not None else rd[:0])
    cfg = O.config_yaml(accum_double=0, trim_ratio=ch.trim_ratio, max_iterations=ch.max_iterations,
                        min_diff_rot=ch.min_diff_rot, min_diff_trans=ch.min_diff_trans, smooth_length=ch.smooth_length)
    rc, T, st, tr = O.icp_compute(cfg, rdf, rf, rn, T16, trace_cap=ch.max_iterations)
    with open(os.path.join(out_dir, "oracle_trace.csv"), "w") as f:
        f.write("iter,limit,n_used," + ",".join("T%d%d" % (r, c) for c in range(4) for r in range(4)) + "\n")
        for k, t in enumerate(tr):
            f.write("%d,%s,%d,%s\n" % (k, g(t["limit"]), t["n_used"], ",".join(g(v) for v in t["T_iter"])))
    Tf = np.asarray(T, np.float32).reshape(4, 4).T
    with open(os.path.join(out_dir, "oracle_result.txt"), "w") as f:
        f.write("rc %d iterations %d converged %d\n" % (rc, st.iterations, st.converged))
        for r in range(4):
            f.write(" ".join(g(Tf[r, c]) for c in range(4)) + "\n")
    with open(os.path.join(out_dir, "README.txt"), "w") as f:
        f.write(("Synthetic HDL-64E drive, LaserTrack::localScanToSubMap's call shape (input filters, sub-map of three scans), "
                 if submap else "Synthetic HDL-64E pair, ") +
                "%d azimuth steps: reading %d points, reference %d points; chain %s\n"
                "(reading_sampling_prob %s, surface normal knn %d ratio %s, trim %s, checkers %d / %s / %s / %d).\n"
                "Written by devtools/dump_for_upstream.py; the float accumulation of libpointmatcher (accum_double 0).\n"
                "Replay on libpointmatcher: INTEGRATION.md, \"Diffing against a real libpointmatcher\".\n\n%s"
                % (n_az, rd.shape[0], ref.shape[0], os.path.relpath(chain_path, ROOT), g(ch.reading_sampling_prob),
                   ch.surface_normal_knn, g(ch.surface_normal_ratio), g(ch.trim_ratio), ch.max_iterations,
                   g(ch.min_diff_rot), g(ch.min_diff_trans), ch.smooth_length,
                   CHOICES + (VOXEL_CHOICES if voxel_grid else "") + (OCTREE_CHOICES if octree_grid else "") + (DENSITY_CHOICES if ch.max_density is not None else "") +
                   (SHADOW_CHOICES if ch.shadow is not None else "") + (COV_SAMPLING_CHOICES if ch.cov_sampling is not None else "") + (MOTION_CHOICES if ch.motion is not None else "")))
    return rc, st.iterations


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--n-az", type=int, default=64)
    ap.add_argument("--chain", default=os.path.join(ROOT, "tests", "golden", "icp_chain.yaml"))
    ap.add_argument("--submap", action="store_true", help="the call shape of LaserTrack::localScanToSubMap (four scans, input filters, three-scan sub-map)")
    ap.add_argument("--voxel-grid", default=None, metavar="VX,VY,VZ[,USE_CENTROID]",
                    help="append VoxelGridDataPointsFilter to the input filter chain and write the chain to OUT_DIR/input_filters.yaml")
    ap.add_argument("--octree-grid", default=None, metavar="MAX_SIZE,MAX_POINT[,SAMPLING_METHOD]",
                    help="append OctreeGridDataPointsFilter to the input filter chain and write the chain to OUT_DIR/input_filters.yaml")
    a = ap.parse_args()
    og = [float(x) for x in a.octree_grid.split(",")] if a.octree_grid else None
    if og is not None and len(og) not in (2, 3):
        ap.error("--octree-grid takes MAX_SIZE,MAX_POINT or MAX_SIZE,MAX_POINT,SAMPLING_METHOD")
    vg = [float(x) for x in a.voxel_grid.split(",")] if a.voxel_grid else None
    if vg is not None and len(vg) not in (3, 4):
        ap.error("--voxel-grid takes VX,VY,VZ or VX,VY,VZ,USE_CENTROID")
    rc, it = dump(a.out_dir, a.n_az, a.chain, a.submap, vg, og)
    print("wrote %s: oracle rc %d, %d iterations" % (a.out_dir, rc, it))
