"""Times ShadowDataPointsFilter, alone and inside compute (DESIGN.md §3 "ShadowDataPointsFilter", §4 "The cost of
ShadowDataPointsFilter").

    python devtools/time_shadow.py [n_az]          (default 16384: the 1 M-point scan pair)

Every call of the C ABI returns after its device work has completed, so the figures are the host's wall time around a
call on clouds that are resident in HBM: median and min..max of 10 calls after 2 warm-up calls.  "the pass" is
lsgpu_icp_filter_shadow on device pointers (two launches of the pass, the scan of the block counts, the total's way to the
host, the wait) on the reference with the normals of SurfaceNormalDataPointsFilter knn 10, and on the reading RandomSampling
0.5 keeps with its normals (knn 7).  "grid of the whole reference" is lsgpu_icp_set_reference on the cloud: what the
SurfaceNormalDataPointsFilter route builds once more than the chain without the module.  "compute" is the handle's compute
on the pair with and without the module, same seed."""
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
    eps = 0.1
    ref, rd, _T_true, T_init = synth.scan_pair(n_az)
    dref, drd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
    print("reference %d points, reading %d points, eps %g" % (len(ref), len(rd), eps))
    with icp.IcpHandle(device=0) as h:
        dn = h.filter_reference_normals(dref, 10)
        print("keep-all normals of the reference, knn 10:", med(lambda: h.filter_reference_normals(dref, 10)))
        kept = {}
        def ref_pass():
            kept["ref"] = len(h.filter_shadow(dref, dn, eps)[0])
        print("the pass, reference:", med(ref_pass), "kept %d of %d" % (kept["ref"], len(ref)))
        drk = h.filter_reading(drd, 0.5, 5)
        drn = torch.from_numpy(h.reading_normals(drk, 7, 1)).cuda()
        def rd_pass():
            kept["rd"] = len(h.filter_shadow(drk, drn, eps)[0])
        print("the pass, reading:", med(rd_pass), "kept %d of %d" % (kept["rd"], len(drk)))
        print("grid of the whole reference (set_reference):", med(lambda: h.set_reference(dref, None)))
    its = {}

    def run(h, name, **kw):
        def f():
            st = h.compute(drd, dref, T_init, 0.5, seed=5, **kw)[1]
            its[name] = (st.iterations, h.info().n_reference)
        print("compute, %s:" % name, med(f), "iterations %d, reference %d points" % its[name])
    with icp.IcpHandle(device=0) as h:
        run(h, "SamplingSurfaceNormal knn 10 ratio 0.5", ssn_knn=10, ssn_ratio=0.5)
        h.set_shadow((None, eps))
        run(h, "SamplingSurfaceNormal + Shadow", ssn_knn=10, ssn_ratio=0.5)
        h.set_shadow(None)
        run(h, "SurfaceNormal knn 10 (keep-all)", ssn_knn=0, sn_knn=10)
        h.set_shadow((None, eps))
        run(h, "SurfaceNormal knn 10 + Shadow", ssn_knn=0, sn_knn=10)
    nc = icp.NormalsConfig(0.6, 7, 1, 1)
    with icp.IcpHandle(device=0, normals=nc) as h:
        run(h, "SamplingSurfaceNormal, reading normals knn 7 + SurfaceNormalOutlierFilter 0.6", ssn_knn=10, ssn_ratio=0.5)
        h.set_shadow((eps, None))
        run(h, "the same + Shadow on the reading", ssn_knn=10, ssn_ratio=0.5)


if __name__ == "__main__":
    main()
