"""dev helper: wall time of CovarianceSamplingDataPointsFilter (lsgpu_icp_filter_cov_sampling) on the 1 M-ray scan of the
benchmark with the normals SurfaceNormalDataPointsFilter gives it, next to its yardstick: SurfaceNormalDataPointsFilter alone
(lsgpu_icp_filter_reference_normals, --knn) on the same cloud and handle.  Median of --reps calls after --warmup calls, the two
alternating, device tensors in and out (each call returns with its work done).  One JSON line per nbSample; the split is the
library's own (lsgpu_icp_cov_sampling_phase_ms, medians over the same calls): sums (three passes, three waits, the Jacobi),
projections + six sorts + heads download, the host walk, picks upload + gather (enqueue; its run time is in the total).
`matches_host_twin`: the module's output against lsgpu_filter_cov_sampling fed the device's sums, bit for bit.
usage: cov_sampling_time.py [--cloud scan.npy] [--n-az 16384] [--reps 50] [--warmup 5] [--knn 10] [--torque-norm 1]
                            [--nb-sample 5000,100000]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from laser_slam_amd import icp, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cloud", default=None, help="(N, 4) float32 .npy; default: the reading of synth.scan_pair(--n-az), the benchmark's scan")
ap.add_argument("--n-az", type=int, default=16384)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--knn", type=int, default=10, help="SurfaceNormalDataPointsFilter's knn")
ap.add_argument("--torque-norm", type=int, default=1)
ap.add_argument("--nb-sample", default="5000,100000")
a = ap.parse_args()
cloud = np.ascontiguousarray(np.load(a.cloud) if a.cloud else synth.scan_pair(a.n_az)[1], np.float32)
d = torch.from_numpy(cloud).cuda()

with icp.IcpHandle() as h:
    normals = h.filter_reference_normals(d, a.knn)
    if not torch.is_tensor(normals):
        normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32)).cuda()
    normals_host = normals.cpu().numpy()
    bad = ~np.isfinite(normals_host).all(axis=1)
    finite = not bool(bad.any())
    if not finite:   # (the module refuses a normal that is not finite: such rows get the z axis, and the JSON says so)
        normals_host[bad] = (0.0, 0.0, 1.0)
        normals = torch.from_numpy(normals_host).cuda()
    for nb in [int(x) for x in a.nb_sample.split(",")]:
        for _ in range(a.warmup):
            h.filter_cov_sampling(d, normals, nb, a.torque_norm)
            h.filter_reference_normals(d, a.knn)
        t_mod, t_sn, phases = [], [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            h.filter_cov_sampling(d, normals, nb, a.torque_norm)
            t_mod.append((time.perf_counter() - t) * 1e3)
            phases.append(h.cov_sampling_phase_ms())
            torch.cuda.synchronize()
            t = time.perf_counter()
            h.filter_reference_normals(d, a.knn)
            t_sn.append((time.perf_counter() - t) * 1e3)
        *got, sums = h.filter_cov_sampling(cloud, normals_host, nb, a.torque_norm, return_sums=True)
        want = icp.cov_sampling(cloud, normals_host, nb, a.torque_norm, sums=sums)
        same = all(np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)) for g, w in zip(got, want))
        ph = np.median(np.array(phases), axis=0)
        print(json.dumps({"points": int(d.shape[0]), "nb_sample": nb, "torque_norm": a.torque_norm, "normals_finite": finite,
                          "module_ms": round(float(np.median(t_mod)), 4), "module_min_ms": round(float(min(t_mod)), 4),
                          "sums_ms": round(float(ph[0]), 4), "project_sort_heads_ms": round(float(ph[1]), 4),
                          "host_walk_ms": round(float(ph[2]), 4), "upload_gather_enqueue_ms": round(float(ph[3]), 4),
                          "surface_normal_knn": a.knn, "surface_normal_ms": round(float(np.median(t_sn)), 4),
                          "surface_normal_min_ms": round(float(min(t_sn)), 4), "matches_host_twin": bool(same),
                          "reps": a.reps, "warmup": a.warmup}))
