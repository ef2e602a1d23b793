"""dev helper: what carrying a scan's normals saves in the call shape of LaserTrack (a new scan against a sub-map of the last
--members scans, everything resident in slots), on --n-az azimuth steps (16384 -> 1 M rays a scan).  Two set-ups, one session:
  (a) module     SurfaceNormalDataPointsFilter knn 10 as the reference filter of every compute: the normals of the whole
                 sub-map are computed at every scan (the only chain a point-to-plane handle could run on slots before)
  (b) carried    the input chain computes every scan's normals once (lsgpu_icp_reading_normals, knn 10, oriented), the slots
                 carry them, the ICP chain has no normals module: assembly with normals + the reading's section pass
Both: RandomSampling 0.5 on the reading, TrimmedDist, point-to-plane; (b) is timed with and without SurfaceNormalOutlierFilter
(the reading's normals travel only with it).  Median wall time of --calls calls after --warmup, and the library's own figure
for the front of a compute (lsgpu_icp_stats.t_reserved[0]: assembly, sections and grid build, up to the loop's start).  One
JSON line per figure, then one with ms per scan of both set-ups and their ratio.  The kernels' own times (k_assemble_submap,
k_cut_pass) are read off a kernel trace of this script, as for every other devtool here (devtools/kernel_times.py)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from laser_slam_amd import icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n-az", type=int, default=16384)
ap.add_argument("--members", type=int, default=3)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

scene = synth.Scene(1234)
poses = [synth.se3(0.8 * i, 0.05 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(2.0 * i)) for i in range(args.members + 1)]
scans = [synth.hdl64_scan(scene, T, args.n_az, 10 + i) for i, T in enumerate(poses)]
# member i in the frame of the last member, the reading guessed a little off its true place
last = poses[args.members - 1]
member_T = [(np.linalg.inv(last) @ poses[i]).astype(np.float32) for i in range(args.members)]
T_init = (np.linalg.inv(last) @ poses[args.members] @ synth.se3(0.05, -0.03, 0, yaw=np.deg2rad(0.3))).astype(np.float32)
SEED, PROB = 7, 0.5


def median_ms(step):
    for _ in range(args.warmup):
        step()
    wall, front = [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        st = step()
        wall.append(1e3 * (time.perf_counter() - t0))
        if st is not None:
            front.append(st.t_reserved[0])
    return float(np.median(wall)), (float(np.median(front)) if front else None)


def report(name, wall, front, **more):
    print(json.dumps(dict(figure=name, wall_ms=round(wall, 4), front_ms=None if front is None else round(front, 4), **more)), flush=True)


out = {}
# ---- (a) the normals module in every compute
with icp.IcpHandle() as h:
    for i in range(args.members):
        h.cloud_upload(1 + i, scans[i])
    h.cloud_upload(0, scans[-1])
    wall, front = median_ms(lambda: h.compute_clouds(0, list(range(1, 1 + args.members)), member_T, T_init, PROB, 0, 0.5, SEED, sn_knn=10)[1])
    report("module_compute", wall, front, points=[len(s) for s in scans])
    out["module_ms_per_scan"] = wall

# ---- (b) normals once per scan, carried
with icp.IcpHandle() as h:
    def normals_once():
        h.reading_normals(scans[-1], 10, 1, (0.0, 0.0, 0.0))
    wall_n, _ = median_ms(normals_once)
    report("carried_normals_once", wall_n, None)
    normals = [h.reading_normals(s, 10, 1, (0.0, 0.0, 0.0)) for s in scans]
for angle in (None, 1.0):
    nrm = None if angle is None else dict(max_angle=angle, reading_normals_given=1)
    with icp.IcpHandle(normals=nrm) as h:
        for i in range(args.members):
            h.cloud_upload(1 + i, scans[i], normals[i])
        h.cloud_upload(0, scans[-1], normals[-1])
        wall, front = median_ms(lambda: h.compute_clouds(0, list(range(1, 1 + args.members)), member_T, T_init, PROB, 0, 0.5, SEED)[1])
        name = "carried_compute" if angle is None else "carried_compute_angle_filter"
        report(name, wall, front)
        out[name + "_ms"] = wall
out["carried_ms_per_scan"] = wall_n + out["carried_compute_ms"]
out["ratio_module_over_carried"] = out["module_ms_per_scan"] / out["carried_ms_per_scan"]
print(json.dumps(dict(figure="per_scan", **{k: round(v, 4) for k, v in out.items()})), flush=True)
