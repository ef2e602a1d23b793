"""Worker of tests/test_select_paths.py: aligns every case of tests/select_cases.py on the device with whatever LSGPU_*
switches the environment carries (they are read once per process) and prints one JSON line: per case and iteration the
limit's bit pattern, the inlier count, A as hex bytes and T_iter; the final T, the iteration count and the retry /
committed counters of lsgpu_icp_stats.  A case whose alignment raises is reported with its error text."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import select_cases as sc
    from laser_slam_amd import icp
    from laser_slam_amd._lib import IcpConfig, LsgpuError, lib
    out = {}
    t0 = time.perf_counter()
    for name in sc.CASES:
        c = sc.case(name)
        cfg = IcpConfig()
        lib().lsgpu_icp_config_yaml(C.byref(cfg))
        for key, v in c["cfg"].items():
            setattr(cfg, key, v)
        with icp.IcpHandle(cfg) as h:
            h.set_reference(c["ref"], c["nrm"])
            try:
                T, st = h.align(c["reading"], c["T_init"])
            except LsgpuError as e:
                out[name] = {"error": str(e), "code": int(e.code)}
                if e.code == 3:     # a HIP error: nothing more is started on this device
                    break
                continue
            tr = h.trace()
        out[name] = {
            "iterations": int(st.iterations), "sel_retries": int(st.pad_), "cap_retries": int(st.cap_retries),
            "committed": int(st.committed_select_iterations),
            "T": [float(v) for v in np.asarray(T, np.float64).ravel()],
            "limit_bits": [sc.bits(t["limit"]) for t in tr], "n_used": [int(t["n_used"]) for t in tr],
            "A": [np.ascontiguousarray(t["A"]).tobytes().hex() for t in tr],
            "T_iter": [[float(v) for v in t["T_iter"]] for t in tr]}
    print("SELECT_RESULT " + json.dumps({"cases": out, "seconds": time.perf_counter() - t0}))


if __name__ == "__main__":
    main()
