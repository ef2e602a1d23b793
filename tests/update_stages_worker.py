"""Worker of tests/test_update_stages.py: the alignments of the 4 k pair whose per-iteration update the test compares
between two processes -- the default (the staged update in the last block of k_normal_eq_loop) and LSGPU_SPLIT_UPDATE=1
(the serial icp_update_lane).  The switches are read once per process, so every case runs in this one.  Prints one line,
UPDATE_STAGES <json>: per case the transform, the iteration count, how it ended and every trace field, as bytes in hex."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    from laser_slam_amd import _lib, icp, synth
    from laser_slam_amd._lib import IcpConfig, lib

    def config(tight=True, max_iterations=None):
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        if tight:   # (long chains: the differential checker's limits of the benchmark)
            cfg.min_diff_rot, cfg.min_diff_trans = 1e-5, 1e-4
        if max_iterations is not None:
            cfg.max_iterations = max_iterations
        return cfg

    # the pair as the generator makes it (reference normals from the product's filter) and as the golden file holds it
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    with icp.IcpHandle(config()) as h:
        rf, rn = h.filter_reference(ref, 10, 1.0, 0)
        rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
    g = np.load(os.path.join(ROOT, "tests", "golden", "icp_pair4k.npz"))
    inputs = {"synth": (rf, rn, rd, T_init),
              "golden": (np.ascontiguousarray(g["ref"]), np.ascontiguousarray(g["nrm"]), np.ascontiguousarray(g["rd"]), g["T_init"])}

    cases = {
        "point_to_plane": dict(cfg=config()),
        "point_to_point": dict(cfg=config(), error_minimizer="PointToPointErrorMinimizer"),
        "force4dof": dict(cfg=config(), motion=icp.MotionConfig(dof=_lib.MOTION_DOF_4)),
        "force2d": dict(cfg=config(), motion=icp.MotionConfig(dof=_lib.MOTION_DOF_3)),
        "robust": dict(cfg=config(), robust=icp.RobustConfig()),
        "by_counter": dict(cfg=config(max_iterations=3)),
        "by_differential": dict(cfg=config(tight=False)),
    }
    out = {}
    for name, kw in cases.items():
        for src, (cref, cnrm, crd, cT) in inputs.items():
            with icp.IcpHandle(**kw) as h:
                h.set_reference(cref, cnrm)
                T, st = h.align(crd, cT)
                tr = h.trace()
                rtr = h.robust_trace() if "robust" in kw else []
            rec = {"T": np.ascontiguousarray(T).tobytes().hex(), "iterations": int(st.iterations), "converged": int(st.converged),
                   "n_trace": len(tr),
                   "robust_trace": [np.float32(t["median"]).tobytes().hex() + np.float32(t["scale"]).tobytes().hex()
                                    + np.float64(t["w_sum"]).tobytes().hex() + str(t["recomputed"]) for t in rtr]}
            for f, dt in (("limit", np.float32), ("n_used", np.int64), ("A", np.float64), ("b", np.float64), ("x", np.float64), ("T_iter", np.float32)):
                rec[f] = [np.ascontiguousarray(t[f], dt).tobytes().hex() for t in tr]
            out[name + "/" + src] = rec
    print("UPDATE_STAGES " + json.dumps(out))


if __name__ == "__main__":
    main()
