"""dev helper: what a scan costs, end to end, on the three ways its normals can reach a point-to-plane compute on slots -- a new
scan against a sub-map of the last --members scans, on --n-az azimuth steps (16384 -> 1 M rays a scan).  One session:
  (a)  module    SurfaceNormalDataPointsFilter knn 10 as the reference filter of every compute (nothing per scan but the upload)
  (b)  composed  lsgpu_icp_reading_normals on the host cloud (knn 10, oriented: a scratch handle, an upload, a download), then
                 lsgpu_cloud_upload_normals, then the compute on carried normals -- the path before lsgpu_cloud_ingest
  (c)  ingest    lsgpu_cloud_ingest (no point module, knn 10, oriented) with the cloud and its normals downloaded, then the
                 same compute
  (c') ingest, download=False: nothing comes back to the host
Every compute: RandomSampling 0.5 on the reading, TrimmedDist, point-to-plane.  Per figure the median wall time of --calls calls after
--warmup; one JSON line per part, then one with ms per scan of the four set-ups and the ratios."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from laser_slam_amd import _lib, icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n-az", type=int, default=16384)
ap.add_argument("--members", type=int, default=3)
ap.add_argument("--calls", type=int, default=15)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

scene = synth.Scene(1234)
poses = [synth.se3(0.8 * i, 0.05 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(2.0 * i)) for i in range(args.members + 1)]
scans = [synth.hdl64_scan(scene, T, args.n_az, 10 + i) for i, T in enumerate(poses)]
last = poses[args.members - 1]
member_T = [(np.linalg.inv(last) @ poses[i]).astype(np.float32) for i in range(args.members)]
T_init = (np.linalg.inv(last) @ poses[args.members] @ synth.se3(0.05, -0.03, 0, yaw=np.deg2rad(0.3))).astype(np.float32)
SEED, PROB, KNN, SENSOR = 7, 0.5, 10, (0.0, 0.0, 0.0)
slots = list(range(1, 1 + args.members))


def median_ms(step):
    for _ in range(args.warmup):
        step()
    wall = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        step()
        wall.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(wall)), float(np.min(wall)), float(np.max(wall))


def report(name, t, **more):
    print(json.dumps(dict(figure=name, median_ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4), **more)), flush=True)
    return t[0]


out = {}
# ---- (a) the normals module in every compute; the scan is uploaded as it is
with icp.IcpHandle() as h:
    for i in range(args.members):
        h.cloud_upload(1 + i, scans[i])

    def module_scan():
        h.cloud_upload(0, scans[-1])
        h.compute_clouds(0, slots, member_T, T_init, PROB, 0, 0.5, SEED, sn_knn=KNN)
    out["a_module_ms"] = report("a_module_upload_and_compute", median_ms(module_scan), points=[len(s) for s in scans])

# ---- (b), (c), (c'): the members carry their normals; what differs is how the new scan gets there
with icp.IcpHandle() as h:
    f = (_lib.PointFilter * 0)()
    for i in range(args.members):
        h.cloud_ingest(1 + i, scans[i], f, -1, KNN, 1, SENSOR, download=False)

    def compute():
        h.compute_clouds(0, slots, member_T, T_init, PROB, 0, 0.5, SEED)

    def composed():
        h.cloud_upload(0, scans[-1], h.reading_normals(scans[-1], KNN, 1, SENSOR))

    def ingest(download):
        h.cloud_ingest(0, scans[-1], f, -1, KNN, 1, SENSOR, download=download)

    def scan_of(front):
        def step():
            front()
            compute()
        return step

    report("b_normals_and_upload", median_ms(composed))
    report("c_ingest_download", median_ms(lambda: ingest(True)))
    report("c_ingest_no_download", median_ms(lambda: ingest(False)))
    report("carried_compute", median_ms(compute))
    out["b_composed_ms"] = report("b_composed_scan", median_ms(scan_of(composed)))
    out["c_ingest_ms"] = report("c_ingest_scan", median_ms(scan_of(lambda: ingest(True))))
    out["c_ingest_no_download_ms"] = report("c_ingest_no_download_scan", median_ms(scan_of(lambda: ingest(False))))
out["ratio_b_over_c"] = out["b_composed_ms"] / out["c_ingest_ms"]
out["ratio_a_over_c"] = out["a_module_ms"] / out["c_ingest_ms"]
out["ratio_b_over_c_no_download"] = out["b_composed_ms"] / out["c_ingest_no_download_ms"]
print(json.dumps(dict(figure="per_scan", **{k: round(v, 4) for k, v in out.items()})), flush=True)
