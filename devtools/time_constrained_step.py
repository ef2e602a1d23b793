"""Times compute with the constrained point-to-plane steps and with BoundTransformationChecker against the free 6-DOF chain
(DESIGN.md §3 "Constrained steps and the bound checker", §4 "The cost of the constrained steps").

    python devtools/time_constrained_step.py [n_az]          (default 16384: the 1 M-point scan pair)

Every call of the C ABI returns after its device work has completed, so the figures are the host's wall time around a
compute on clouds that are resident in HBM, same seed: median and min..max of 10 calls after 2 warm-up calls.  The chains
differ in what they converge to and in how many iterations they take, so the time per iteration is printed beside the
total.  The pair's true motion has 0.2 degrees of pitch that the constrained steps cannot follow: their iteration counts are
those of that pair, not a property of the steps."""
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
    return float(np.median(ts)), "%.3f ms (%.3f .. %.3f)" % (np.median(ts), min(ts), max(ts))


def main():
    import torch
    from laser_slam_amd import _lib, icp, synth
    n_az = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    ref, rd, _T_true, T_init = synth.scan_pair(n_az)
    dref, drd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
    print("reference %d points, reading %d points" % (len(ref), len(rd)))
    rows = (("6-DOF", None), ("force4DOF", dict(dof=_lib.MOTION_DOF_4)), ("force2D", dict(dof=_lib.MOTION_DOF_3)),
            ("6-DOF + BoundTransformationChecker 1 rad / 5 m", dict(bound=True, max_rotation_norm=1.0, max_translation_norm=5.0)))
    for chain_name, kw in (("Trimmed 0.75", {}), ("Trimmed 0.75 + matcher maxDist 2 + MedianDist 3", dict(matcher_max_dist=2.0, outlier_median_factor=3.0))):
        with icp.IcpHandle(device=0, **kw) as h:
            for name, motion in rows:
                h.set_motion(motion)
                its = {}

                def f():
                    its["n"] = h.compute(drd, dref, T_init, 0.5, 10, 0.5, seed=5)[1].iterations
                m, text = med(f)
                print("compute, %s, %s: %s, %d iterations, %.3f ms per iteration" % (chain_name, name, text, its["n"], m / max(its["n"], 1)))


if __name__ == "__main__":
    main()
