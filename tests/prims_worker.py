"""Worker of tests/test_primitive_sizes.py: the radix sort under a forced LSGPU_SORT_ITEMS (read once per process).  At
every size of prim_cases.forced_sizes(ITEMS) it runs, on one handle, filter_voxel_grid with both leaves against
oracle.voxel_grid, apply_point_filters with VoxelGridDataPointsFilter against ref_voxel_grid, and set_reference + knn of a
reading of the same size against tests/cpp/knn_brute.c (prim_cases has the checks), and prints one JSON line per size:
PRIM_RESULT {"n", "failures", "seconds"} -- or {"n", "error", "code"} for a call that raised; after a HIP error nothing more
is started.  The last line is PRIM_DONE {"items", "sizes", "seconds"}."""
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
    import prim_cases as pc
    from laser_slam_amd import icp
    from laser_slam_amd._lib import HIP_ERROR, LsgpuError
    from oracle import oracle_py as oracle
    items = int(os.environ["LSGPU_SORT_ITEMS"])
    sizes = pc.forced_sizes(items)
    t0 = time.perf_counter()
    done = []
    with tempfile.TemporaryDirectory() as tmp, icp.IcpHandle() as h:
        brute = host_loop.build_brute(tmp)
        for n in sizes:
            t = time.perf_counter()
            cloud, side = pc.uniform_cloud(n)
            query = pc.uniform_cloud(n, seed=1)[0]
            try:
                f = pc.pcl_voxel_check(oracle, h, cloud, side, full=n >= 4096)
                f += pc.chain_voxel_check(h, cloud, side)
                f += pc.knn_check(oracle, brute, h, cloud, query)
                res = {"n": n, "failures": f, "seconds": time.perf_counter() - t}
            except LsgpuError as e:
                res = {"n": n, "error": str(e), "code": int(e.code)}
            print("PRIM_RESULT " + json.dumps(res), flush=True)
            done.append(n)
            if res.get("code") == HIP_ERROR:     # nothing more is started on this device
                break
    print("PRIM_DONE " + json.dumps({"items": items, "sizes": done, "seconds": time.perf_counter() - t0}), flush=True)


if __name__ == "__main__":
    main()
