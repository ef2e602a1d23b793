"""dev helper: what KDTreeMatcher knn = k costs on the configs[1] workload (the 1 M-point pair of bench.py,
synth.scan_pair(16384), chain of icp_default.yaml): the whole lsgpu_icp_compute in ms and the median search launch
(k = 1: k_knn_tile / k_knn_cone + fallback; k >= 2: k_knnk_seed + k_knnk_tile + k_knnk_fallback) for knn 1, 3 and 8.

    python devtools/knn_k_times.py [REPS]

Compute times: REPS calls per k after one warm-up call, median, profile_kernels = 0.  Search times: one more call with
profile_kernels = 1 (HIP events around every search, from the per-iteration trace), median over its iterations."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(reps):
    import numpy as np
    import torch
    from laser_slam_amd import icp, synth
    from laser_slam_amd._lib import IcpConfig, lib
    ref, rd, T_true, T_init = synth.scan_pair(16384)
    dref, drd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
    for k in (1, 3, 8):
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        cfg.matcher_knn = k
        with icp.IcpHandle(cfg) as h:
            T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)      # warm-up (allocations, first launches)
            ms = []
            for _ in range(reps):
                T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                ms.append(st.t_total_ms)
        cfg.profile_kernels = 1
        with icp.IcpHandle(cfg) as h:
            h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
            h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
            us = sorted(t["knn_main_us"] + t["knn_fallback_us"] for t in h.trace())
        dt, dr = synth.pose_error(T.astype(np.float64), T_true)
        print(f"knn {k}: compute median {np.median(ms):.2f} ms (min {min(ms):.2f}) over {reps}, {st.iterations} iterations, "
              f"final_n_used {st.final_n_used}, search median {us[len(us) // 2]:.1f} us (max {us[-1]:.1f} us), "
              f"|dt| {dt:.2e} m |dr| {dr:.2e} rad")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
