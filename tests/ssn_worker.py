"""Worker of tests/test_reference_filter_shapes.py: the device reference filter under whatever LSGPU_SSN_ROOT /
LSGPU_SSN_SORT_LEVELS the environment carries (read once per process).  On one handle it walks the table of
ssn_cases.sizes(B, knn) for B = LSGPU_SSN_ROOT (2048 without it: what the library takes by itself at these sizes), every
knn of ssn_cases.KNNS and the three clouds, and compares with the oracle, uint32 views, nothing left out:
  filter_reference(cloud, knn, 1.0, seed)                        points, order, normals
  filter_reference(cloud, knn, 0.4, seed), filter_reading(cloud, 0.5, -1) right after it: the oracle's filter and its
      random_sampling(n, 0.5, -1) continuing the oracle's stream (every knn on every cloud: a worker takes seconds)
  device pointers in and out at B + 1 (knn 10, `quantised`)
and prints one JSON line per case: SSN_RESULT {"b", "n", "knn", "kind", "shape", "kept", "failures", "seconds"} -- or
{..., "error", "code"} for a call that raised; after a HIP error nothing more is started.  The last line is
SSN_DONE {"b", "sort_levels", "cases", "calls", "ssn_calls", "ssn_sort_fallbacks", "seconds"}."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 2


def check(oracle, h, sc, b, n, knn, kind, calls):
    """One case -> (kept at ratio 1, failures in words); calls[0] counts the filter_reference calls made"""
    import numpy as np
    f = []
    p = sc.cloud(kind, n)
    of, on = oracle.sampling_surface_normal(p, knn, 1.0, SEED)
    calls[0] += 1
    gf, gn = h.filter_reference(p, knn, 1.0, SEED)
    if not (sc.same(gf, of) and sc.same(gn, on)):
        f.append("ratio 1: %d points for the oracle's %d, or other bits" % (len(gf), len(of)))
    # ratio 0.4: a point's draw is the one of its place in the traversal, so the order INSIDE a box decides who is kept
    seed = 3 + n % 89
    of4, on4 = oracle.sampling_surface_normal(p, knn, 0.4, seed)
    ok = oracle.random_sampling(n, 0.5, -1)
    calls[0] += 1
    gf4, gn4 = h.filter_reference(p, knn, 0.4, seed)
    gr = h.filter_reading(p, 0.5, -1)
    if not (sc.same(gf4, of4) and sc.same(gn4, on4)):
        f.append("ratio 0.4: %d points for the oracle's %d, or other bits" % (len(gf4), len(of4)))
    if not sc.same(np.ascontiguousarray(gr), p[ok]):
        f.append("the draw stream stands elsewhere after ratio 0.4: filter_reading keeps %d points for the oracle's %d, or others" % (len(gr), len(ok)))
    if n == b + 1 and knn == sc.DEVICE_POINTER_KNN and kind == "quantised":
        import torch
        d = torch.from_numpy(p).cuda()
        calls[0] += 1
        tf, tn = h.filter_reference(d, knn, 1.0, SEED)
        if not (tf.is_cuda and tn.is_cuda and sc.same(tf.cpu().numpy(), of) and sc.same(tn.cpu().numpy(), on)):
            f.append("device pointers: %d points for the oracle's %d, or other bits" % (len(tf), len(of)))
        if d.cpu().numpy().tobytes() != p.tobytes():
            f.append("device pointers: the input was written")
    return len(of), f


def main():
    import ssn_cases as sc
    from laser_slam_amd import icp
    from laser_slam_amd._lib import HIP_ERROR, LsgpuError
    from oracle import oracle_py as oracle
    oracle.lib()
    b = int(os.environ.get("LSGPU_SSN_ROOT", sc.ROOTS[0]))
    t0 = time.perf_counter()
    calls, cases, stop = [0], 0, False
    with icp.IcpHandle() as h:
        for knn in sc.KNNS:
            for n in sc.sizes(b, knn):
                assert sc.root_auto(n) == sc.ROOTS[0]
                for kind in sc.KINDS:
                    t = time.perf_counter()
                    res = {"b": b, "n": n, "knn": knn, "kind": kind, "shape": sc.brief(sc.shape(n, knn, b))}
                    try:
                        res["kept"], res["failures"] = check(oracle, h, sc, b, n, knn, kind, calls)
                        res["seconds"] = time.perf_counter() - t
                    except LsgpuError as e:
                        res["error"], res["code"] = str(e), int(e.code)
                    print("SSN_RESULT " + json.dumps(res), flush=True)
                    cases += 1
                    if res.get("code") == HIP_ERROR:     # nothing more is started on this device
                        stop = True
                        break
                if stop:
                    break
            if stop:
                break
        pi = None if stop else h.policy_info()
    done = {"b": b, "sort_levels": "LSGPU_SSN_SORT_LEVELS" in os.environ, "cases": cases, "calls": calls[0], "seconds": time.perf_counter() - t0}
    if pi is not None:
        done["ssn_calls"], done["ssn_sort_fallbacks"] = int(pi.ssn_calls), int(pi.ssn_sort_fallbacks)
    print("SSN_DONE " + json.dumps(done), flush=True)


if __name__ == "__main__":
    main()
