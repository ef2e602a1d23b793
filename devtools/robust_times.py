"""dev helper: what RobustOutlierFilter costs on the configs[1] workload (the 1 M-point pair of bench.py,
synth.scan_pair(16384), reading filter 0.5, reference filter knn 10) against the nearest existing plan, a
MedianDistOutlierFilter chain (it too runs two selects per iteration): the whole lsgpu_icp_compute in ms, and per
iteration the search, the selects (for cauchy / mad: the trim select, the median's and the MAD's three passes) and the
normal-equation pass (weighted for the robust chain).

    python devtools/robust_times.py [REPS]

Rows: MedianDist factor 3 | cauchy / mad | cauchy / none (no MAD passes: what the weighted pass alone costs) |
cauchy / mad nbIterationForScale 3 (MAD passes in three iterations only).  Compute times: REPS calls after one warm-up
call, median, profile_kernels = 0.  Per-iteration times: one more handle with profile_kernels = 1 (HIP events around the
search, the selects and the normal equations of every iteration), second call; the MAD passes' share is the difference of
the select time between the mad and the none rows."""
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
    rows = [("MedianDist factor 3", dict(outlier_median_factor=3.0), None),
            ("cauchy / mad", {}, dict(robust_fct="cauchy")),
            ("cauchy / none", {}, dict(robust_fct="cauchy", scale_estimator="none", tuning=0.1)),
            ("cauchy / mad, nbIterationForScale 3", {}, dict(robust_fct="cauchy", nb_iteration_for_scale=3))]
    for name, fields, rb in rows:
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        cfg.trim_ratio = 1.0
        for k, v in fields.items():
            setattr(cfg, k, v)
        with icp.IcpHandle(cfg, robust=rb) as h:
            T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)      # warm-up (allocations, first launches)
            ms = []
            for _ in range(reps):
                T, st = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
                ms.append(st.t_total_ms)
        cfg.profile_kernels = 1
        with icp.IcpHandle(cfg, robust=rb) as h:
            h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
            _T, stp = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=1)
        n = max(1, stp.knn_launches)
        dt, dr = synth.pose_error(T.astype(np.float64), T_true)
        per_it = (st.t_total_ms - st.t_reserved[0]) / max(1, st.iterations)
        print(f"{name}: compute median {np.median(ms):.2f} ms (min {min(ms):.2f}) over {reps}, {st.iterations} iterations, "
              f"loop {per_it * 1e3:.0f} us per iteration; profiled: search {stp.t_knn_ms / n * 1e3:.1f} us + selects "
              f"{stp.t_select_ms / n * 1e3:.1f} us + normal eq. {stp.t_ne_ms / n * 1e3:.1f} us per iteration; final_n_used {st.final_n_used}, "
              f"|dt| {dt:.2e} m |dr| {dr:.2e} rad", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
