"""Worker of tests/test_reading_sizes.py: aligns the readings of size_cases.WORKER_SIZES on the device with whatever
LSGPU_* switches the environment carries (LSGPU_NE_BLOCKS is read once per process), runs each through
size_cases.device_case -- the oracle, the numpy model fed the device's own poses, a second alignment -- and prints one
JSON line: per size the facts of that check.  A size whose alignment raises is reported with its error text; after a HIP
error nothing more is started."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import host_loop
    import size_cases as sz
    from laser_slam_amd import icp
    from laser_slam_amd._lib import LsgpuError
    from oracle import oracle_py as oracle
    out = {}
    t0 = time.perf_counter()
    n_big = len(sz.scans(sz.WORKER_AZ)[1])     # (the largest case needs at least 131 073 points: the parent asserts it)
    with tempfile.TemporaryDirectory() as tmp, icp.IcpHandle() as h:
        rf, rn = sz.reference(oracle)
        h.set_reference(rf, rn)
        model = sz.Model(oracle, host_loop.build_brute(tmp), rf, rn, h.reference_mean())
        for n in sz.WORKER_SIZES:
            try:
                out[str(n)] = sz.device_case(oracle, model, h, n, sz.worker_az(n))
            except LsgpuError as e:
                out[str(n)] = {"error": str(e), "code": int(e.code)}
                if e.code == 3:     # a HIP error: nothing more is started on this device
                    break
    print("SIZE_RESULT " + json.dumps({"cases": out, "blocks": os.environ.get("LSGPU_NE_BLOCKS"), "big_reading": n_big,
                                       "seconds": time.perf_counter() - t0}))


if __name__ == "__main__":
    main()
