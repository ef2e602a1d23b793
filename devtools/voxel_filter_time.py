"""dev helper: wall time of VoxelGridDataPointsFilter in the input filter chain (lsgpu_apply_point_filters with this one
module) on the 1 M-ray scan of the benchmark, next to its yardstick: pcl::VoxelGrid (lsgpu_filter_voxel_grid, min_points 1)
on the same cloud, leaf and handle -- the two share the sort and the scan; the module adds a bounds pass with a read-back
and a scatter.  Median of --reps calls after --warmup calls, the two alternating, device tensor in and out (each call returns with its work
done).  One JSON line per voxel size; `matches_host_twin`: the module's output at this size against
lsgpu_filter_voxel_grid_points, bit for bit.
usage: voxel_filter_time.py [--cloud scan.npy] [--n-az 16384] [--reps 200] [--warmup 20]"""
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
    for leaf in (0.1, 0.5):
        chain = (_lib.PointFilter * 1)()
        chain[0].type, chain[0].flag, chain[0].dim = _lib.FILTER_VOXEL_GRID, 1, 0
        for i in range(3):
            chain[0].v[i] = leaf
        (mod_ms, mod_min, mod_n), (pcl_ms, pcl_min, pcl_n) = clock_pair(lambda: h.apply_point_filters(chain, d),
                                                                        lambda: h.filter_voxel_grid(d, leaf, 1))
        same = np.array_equal(h.apply_point_filters(chain, d).cpu().numpy().view(np.uint32),
                              icp.voxel_grid_points(cloud, (leaf, leaf, leaf), 1).view(np.uint32))
        print(json.dumps({"points": int(d.shape[0]), "vsize": leaf, "voxel_grid_module_ms": round(mod_ms, 4),
                          "voxel_grid_module_min_ms": round(mod_min, 4), "module_points_out": mod_n,
                          "pcl_voxel_grid_ms": round(pcl_ms, 4), "pcl_voxel_grid_min_ms": round(pcl_min, 4),
                          "pcl_points_out": pcl_n, "ratio": round(mod_ms / pcl_ms, 3), "matches_host_twin": bool(same), "reps": a.reps, "warmup": a.warmup}))
