"""dev helper: wall time of OctreeGridDataPointsFilter in the input filter chain (lsgpu_apply_point_filters with this one
module) on the 1 M-ray scan of the benchmark, next to its yardstick: VoxelGridDataPointsFilter (--vsize, centroids) on the same
cloud and handle -- both are a 64-bit stable sort plus streaming passes; the octree sorts 3 x depth path bits instead of
the voxel index's, and sorts a second time (the leaf ranks, from input order) to put every leaf in ascending input index.
Median of --reps calls after --warmup calls, the two alternating, device tensor in and out (each call returns with its work
done).  One JSON line per octree setting; `matches_host_twin`: the module's output at this setting against
lsgpu_filter_octree_grid_points, bit for bit.
usage: octree_filter_time.py [--cloud scan.npy] [--n-az 16384] [--reps 200] [--warmup 20] [--vsize 0.5] [--method 0]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from laser_slam_amd import _lib, icp, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", default=None, help="(N, 4) float32 .npy; default: the reading of synth.scan_pair(--n-az), the benchmark's scan")
ap.add_argument("--n-az", type=int, default=16384)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--vsize", type=float, default=0.5, help="the voxel module's vSizeX = vSizeY = vSizeZ")
ap.add_argument("--method", type=int, default=0, help="samplingMethod: 0 FirstPts, 1 RandomPts, 2 Centroid, 3 Medoid")
a = ap.parse_args()
cloud = np.load(a.cloud) if a.cloud else synth.scan_pair(a.n_az)[1]
d = torch.from_numpy(np.ascontiguousarray(cloud, np.float32)).cuda()


def clock_pair(call_a, call_b):
    """The two calls alternate, so that whatever else the host does falls on both alike."""
    for _ in range(a.warmup):
        out_a, out_b = call_a(), call_b()
    ta, tb = [], []
    for _ in range(a.reps):
        for call, ts in ((call_a, ta), (call_b, tb)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t) * 1e3)
    return (float(np.median(ta)), float(min(ta)), int(out_a.shape[0])), (float(np.median(tb)), float(min(tb)), int(out_b.shape[0]))


with icp.IcpHandle() as h:
    voxel = (_lib.PointFilter * 1)()
    voxel[0].type, voxel[0].flag, voxel[0].dim = _lib.FILTER_VOXEL_GRID, 1, 0
    for i in range(3):
        voxel[0].v[i] = a.vsize
    for max_size, max_point in ((0.0, 1), (0.5, 1)):
        chain = (_lib.PointFilter * 1)()
        chain[0].type, chain[0].dim, chain[0].flag = _lib.FILTER_OCTREE_GRID, a.method, 1
        chain[0].v[0], chain[0].v[1] = max_size, max_point
        (oct_ms, oct_min, oct_n), (vox_ms, vox_min, vox_n) = clock_pair(lambda: h.apply_point_filters(chain, d, seed=1),
                                                                        lambda: h.apply_point_filters(voxel, d))
        same = np.array_equal(h.apply_point_filters(chain, d, seed=1).cpu().numpy().view(np.uint32),
                              icp.octree_grid_points(cloud, max_size, max_point, a.method, 1).view(np.uint32))
        print(json.dumps({"points": int(d.shape[0]), "max_size_by_node": max_size, "max_point_by_node": max_point, "sampling_method": a.method,
                          "octree_grid_module_ms": round(oct_ms, 4), "octree_grid_module_min_ms": round(oct_min, 4), "octree_points_out": oct_n,
                          "vsize": a.vsize, "voxel_grid_module_ms": round(vox_ms, 4), "voxel_grid_module_min_ms": round(vox_min, 4),
                          "voxel_points_out": vox_n, "ratio": round(oct_ms / vox_ms, 3), "matches_host_twin": bool(same),
                          "reps": a.reps, "warmup": a.warmup}))
