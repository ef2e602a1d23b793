"""Worker of tests/test_direction_index.py: every case of tests/cone_cases.py (or those named on the command line) at both
trim ratios, under whatever LSGPU_* switches the environment carries (they are read once per process).  One line per case:
everything the alignments return, the floating-point words as hex so that the parent compares bits."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _hex(a, dtype):
    import numpy as np
    return np.ascontiguousarray(a, dtype).tobytes().hex()


def main():
    import numpy as np
    import cone_cases as cc
    from laser_slam_amd import icp
    from laser_slam_amd._lib import IcpConfig, lib
    names = sys.argv[1:] or cc.CASES
    handles = {}
    for ratio in cc.RATIOS:
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        cfg.min_diff_rot, cfg.min_diff_trans, cfg.trim_ratio = cc.MIN_DIFF_ROT, cc.MIN_DIFF_TRANS, ratio
        handles[ratio] = icp.IcpHandle(cfg)
    try:
        for name in names:
            c = cc.case(name)
            out = {"case": name, "runs": {}}
            for ratio, h in handles.items():
                h.set_reference(c["ref"], c["nrm"])
                T, st = h.align(c["rd"], c["T_init"])
                tr = h.trace()
                out["runs"][repr(ratio)] = {
                    "T": _hex(T, np.float32), "iterations": int(st.iterations), "converged": int(st.converged),
                    "limit": [_hex(t["limit"], np.float32) for t in tr], "n_used": [int(t["n_used"]) for t in tr],
                    "A": [_hex(t["A"], np.float64) for t in tr], "b": [_hex(t["b"], np.float64) for t in tr],
                    "T_iter": [_hex(t["T_iter"], np.float32) for t in tr],
                    "stragglers": [int(t["stragglers"]) for t in tr],
                    "cap_retries": int(st.cap_retries), "launches": int(st.direction_index_launches), "occupancy": float(st.direction_index_occupancy),
                    "heavy_share": float(st.direction_index_heavy_share)}
            print("CONE_RESULT " + json.dumps(out), flush=True)
    finally:
        for h in handles.values():
            h.close()


if __name__ == "__main__":
    main()
