"""dev helper: per-launch time of the loop's normal-equation kernel, point-to-plane (k_normal_eq_loop<0>) against
point-to-point (k_normal_eq_loop<1>), on the configs[1] workload (the 1 M-point pair of bench.py, chain F reference).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python devtools/p2p_kernel_times.py
    python devtools/p2p_kernel_times.py --parse OUT

The workload aligns the same reading against the same reference with both minimizers (point-to-point without normals),
REPS times each.  The parser takes every launch of the two instantiations from the kernel trace and reports the median of
those that did work (launches enqueued behind the loop's end exit at once: < 8 us).  Under LSGPU_SPLIT_UPDATE=1 the update
lane is a launch of its own (k_icp_update<0> / <1>) and is reported as well."""
import csv
import ctypes as C
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5


def run():
    import numpy as np
    import torch
    from laser_slam_amd import icp, synth
    from laser_slam_amd._lib import IcpConfig, lib
    ref, rd, T_true, T_init = synth.scan_pair(16384)
    cfg = IcpConfig()
    lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.min_diff_rot, cfg.min_diff_trans = 1e-5, 1e-4        # configs[1]'s checker, as bench.py
    with icp.IcpHandle(cfg) as hf:
        dref, dn = hf.filter_reference(torch.from_numpy(ref).cuda(), 10, 1.0, 0)
    drd = torch.from_numpy(rd).cuda()
    for name, minimizer, nrm in (("point-to-plane", "PointToPlaneErrorMinimizer", dn),
                                 ("point-to-point", "PointToPointErrorMinimizer", None)):
        with icp.IcpHandle(cfg, 0, minimizer) as h:
            h.set_reference(dref, nrm)
            for _ in range(REPS):
                T, st = h.align(drd, T_init)
            dt, dr = synth.pose_error(T.astype(np.float64), T_true)
            print(f"{name}: {st.iterations} iterations, {st.t_total_ms:.3f} ms per align, |dt| {dt:.2e} m |dr| {dr:.2e} rad")


def parse(out_dir):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    # (LSGPU_SPLIT_UPDATE=1: the update lane runs as its own launch, k_icp_update<MIN>, and its time shows on its own)
    for inst, floor in (("k_normal_eq_loop<0>", 8.0), ("k_normal_eq_loop<1>", 8.0), ("k_icp_update<0>", 3.0), ("k_icp_update<1>", 3.0)):
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if inst in r["Kernel_Name"])
        if not d:
            continue
        busy = [x for x in d if x >= floor]
        med = busy[len(busy) // 2] if busy else float("nan")
        print(f"{inst}: {len(d)} launches, {len(busy)} that did work, median {med:.2f} us, min {busy[0] if busy else float('nan'):.2f} us")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        run()
