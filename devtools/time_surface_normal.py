"""Times SurfaceNormalDataPointsFilter alone and inside compute ("Surface normals of every point").

    python devtools/time_surface_normal.py [n_az]          (default 16384: the 1 M-point scan pair)

Every call of the C ABI returns after its device work has completed, so the figures are the host's wall time around a
call on clouds that are resident in HBM: median and min..max of 10 calls after 2 warm-up calls.  "filter" is
lsgpu_icp_filter_reference_normals = set_reference's grid build + the search and normal kernels + the copy of the normals
into caller order; "grid" is lsgpu_icp_set_reference alone on the same cloud, so filter - grid is what the new kernels
cost.  "compute" is ICP.compute on the pair with each reference filter, same seed, same commit."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(f, n=10, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(n):
        t = time.perf_counter(); f(); ts.append((time.perf_counter() - t) * 1e3)
    return "%.3f ms (%.3f .. %.3f)" % (np.median(ts), min(ts), max(ts))


def main():
    import torch
    from laser_slam_amd import icp, synth
    n_az = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    ref, rd, _T_true, T_init = synth.scan_pair(n_az)
    dref, drd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
    print("reference %d points, reading %d points" % (len(ref), len(rd)))
    with icp.IcpHandle(device=0) as h:
        print("grid (set_reference, no normals):", med(lambda: h.set_reference(dref, None)))
        for knn in (5, 10, 20):
            print("filter knn %2d:" % knn, med(lambda: h.filter_reference_normals(dref, knn)))
        its = {}
        def run(name, **kw):
            def f():
                its[name] = h.compute(drd, dref, T_init, 0.5, seed=5, **kw)[1].iterations
            print("compute, %s:" % name, med(f), "iterations", its[name])
        run("SamplingSurfaceNormal knn 10 ratio 0.5", ssn_knn=10, ssn_ratio=0.5)
        run("SurfaceNormal knn 10", ssn_knn=0, sn_knn=10)
        run("SurfaceNormal knn 5", ssn_knn=0, sn_knn=5)


if __name__ == "__main__":
    main()
