"""dev helper: what KDTreeMatcher maxDist costs on the configs[1] workload (the 1 M-point pair of bench.py,
synth.scan_pair(16384), chain of icp_default.yaml) for knn 1 and 3 with maxDist absent, 100 m (the chain plan with a bound
that cuts nothing), 1.0 m and 0.3 m: the whole lsgpu_icp_compute in ms, the median search of an iteration, the first two
searches, and the share of the reading that goes to the wave-per-query fallback (k_knnk_fallback) per iteration.

    python devtools/chain_times.py [REPS]

maxDist absent is the plan the handle had before (knn 1: the one-neighbour loop; knn 3: the k-match plan); any finite
maxDist puts the handle on the chain plan (lsgpu_policy.h: k-best search bounded by maxDist, full select every iteration).
Compute times: REPS calls after one warm-up call, median, profile_kernels = 0.  Search times: one more handle with
profile_kernels = 1 (HIP events around every search, from the per-iteration trace), second call."""
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
    for k in (1, 3):
        for max_dist in (0.0, 100.0, 1.0, 0.3):
            cfg = IcpConfig()
            lib().lsgpu_icp_config_yaml(C.byref(cfg))
            cfg.matcher_knn = k
            cfg.matcher_max_dist = max_dist
            with icp.IcpHandle(cfg) as h:
                T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)      # warm-up (allocations, first launches)
                ms = []
                for _ in range(reps):
                    T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                    ms.append(st.t_total_ms)
            cfg.profile_kernels = 1
            with icp.IcpHandle(cfg) as h:
                h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                _T, stp = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                tr = h.trace()
                us = [t["knn_main_us"] + t["knn_fallback_us"] for t in tr]
                strag = [int(t["stragglers"]) for t in tr]
            n_reading = 0.5 * len(rd)                                           # (the reading filter keeps about half)
            dt, dr = synth.pose_error(T.astype(np.float64), T_true)
            first = " ".join(f"{u:.0f}" for u in us[:2])
            print(f"knn {k} maxDist {max_dist if max_dist else 'absent'}: compute median {np.median(ms):.2f} ms (min {min(ms):.2f}) "
                  f"over {reps}, {st.iterations} iterations, final_n_used {st.final_n_used}, search median "
                  f"{sorted(us)[len(us) // 2]:.1f} us (max {max(us):.1f}), first two {first} us, select {stp.t_select_ms / max(1, stp.knn_launches) * 1e3:.1f} us "
                  f"+ normal eq. {stp.t_ne_ms / max(1, stp.knn_launches) * 1e3:.1f} us per iteration, fallback share per iteration "
                  f"first {strag[0] / n_reading:.3f} median {sorted(strag)[len(strag) // 2] / n_reading:.3f}, "
                  f"|dt| {dt:.2e} m |dr| {dr:.2e} rad", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
