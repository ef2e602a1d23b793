"""dev helper: what SurfaceNormalOutlierFilter, the reading's normals and the orientation pairs cost on the configs[1]
workload (the 1 M-point pair of bench.py, synth.scan_pair(16384), reading filter 0.5, reference filter knn 10) against the
chain they sit on, TrimmedDist 0.75 + KDTreeMatcher maxDist 1.0 (the chain plan): the whole lsgpu_icp_compute in ms, the
time in front of the loop (filters, grids, reading normals: stats.t_reserved[0]) and per iteration the search, the select
and the normal-equation pass.

    python devtools/normal_outlier_times.py [REPS]

Rows: the parent's chain | + angle filter with reading normals (knn 7) | + orientation on both sides | the parent's chain
with LSGPU_NO_SIDE_STREAM=1 in a child process (what the lost side-stream overlap alone costs: a chain with reading
normals runs on one stream).  The reading-normal step is the difference of the time in front of the loop between row 2 and
row 4.  Compute times: REPS calls after one warm-up call, median, profile_kernels = 0.  Per-iteration times: one more
handle with profile_kernels = 1, second call."""
import ctypes as C
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(reps, only_plain=False):
    import numpy as np
    import torch
    from laser_slam_amd import icp, synth
    from laser_slam_amd._lib import IcpConfig, lib
    ref, rd, T_true, T_init = synth.scan_pair(16384)
    dref, drd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
    rows = [("Trimmed 0.75 + maxDist 1.0" + (" (one stream)" if only_plain else ""), None)]
    if not only_plain:
        rows += [("+ SurfaceNormalOutlierFilter 1.57, reading normals knn 7", dict(max_angle=1.57, reading_sn_knn=7)),
                 ("+ orientation on both sides", dict(max_angle=1.57, reading_sn_knn=7, reading_orient=1, reference_orient=1))]
    for name, normals in rows:
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        cfg.matcher_max_dist = 1.0
        with icp.IcpHandle(cfg, normals=normals) as h:
            T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)      # warm-up (allocations, first launches)
            ms, front = [], []
            for _ in range(reps):
                T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                ms.append(st.t_total_ms)
                front.append(st.t_reserved[0])
            rej = h.normal_angle_trace()
        cfg.profile_kernels = 1
        with icp.IcpHandle(cfg, normals=normals) as h:
            h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
            _T, stp = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
        n = max(1, stp.knn_launches)
        dt, dr = synth.pose_error(T.astype(np.float64), T_true)
        print(f"{name}: compute median {np.median(ms):.2f} ms (min {min(ms):.2f}) over {reps}, in front of the loop "
              f"{np.median(front):.2f} ms, {st.iterations} iterations; profiled: search {stp.t_knn_ms / n * 1e3:.1f} us + select "
              f"{stp.t_select_ms / n * 1e3:.1f} us + normal eq. {stp.t_ne_ms / n * 1e3:.1f} us per iteration; final_n_used "
              f"{st.final_n_used}, rejected by the angle test in iteration 1: {rej[0]['rejected'] if rej else 0}, "
              f"|dt| {dt:.2e} m |dr| {dr:.2e} rad", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "plain":
        main(int(sys.argv[1]), only_plain=True)
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
        main(reps)
        env = dict(os.environ, LSGPU_NO_SIDE_STREAM="1")      # a fresh process: the switch is read once
        subprocess.check_call([sys.executable, os.path.abspath(__file__), str(reps), "plain"], env=env)
