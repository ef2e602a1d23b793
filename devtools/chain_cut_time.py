"""dev helper: what a cut section costs (MaxDist-, MinDist-, BoundingBox-, RemoveNaNDataPointsFilter in the ICP chain's filter
sections, lsgpu_icp_set_chain_cuts) on the benchmark's 1 M-point pair, clouds resident in HBM.  Median of --calls calls (200)
after --warmup, one JSON line per figure:
  compute_cuts        lsgpu_icp_compute with MinDist + MaxDist + BoundingBox on both sides through set_chain_cuts (one pass a section)
  compute_sequential  the only route before: lsgpu_apply_point_filters on both clouds (a launch chain and a readback per module),
                      then lsgpu_icp_compute on what they leave
  compute_plain       lsgpu_icp_compute without cut modules (the whole clouds)
  section_N           lsgpu_icp_filter_section alone with N = 1, 3, 8 modules against lsgpu_apply_point_filters with the same modules
Wall time on a plain handle; with a profile_kernels handle also the library's own figures (lsgpu_icp_stats: t_total_ms, the
filters + grid part t_reserved[0], the kNN / select / normal-equation kernel times from HIP events)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from laser_slam_amd import _lib, icp, synth

ap = argparse.ArgumentParser()
ap.add_argument("--n-az", type=int, default=16384, help="azimuth steps (16384 -> 1 M rays, bench.py's pair)")
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--section-warmup", type=int, default=100, help="calls in front of every timed series of a section alone (they are ~50 us each)")
ap.add_argument("--only", choices=("all", "compute", "sections"), default="all")
args = ap.parse_args()

ref, rd, T_true, T_init = synth.scan_pair(args.n_az, noise_seeds=(1, 2), guess_seed=7)     # bench.py's pair (rank 0)
d_ref, d_rd = torch.from_numpy(ref).cuda(), torch.from_numpy(rd).cuda()
torch.cuda.synchronize()

MODS = [(2, -1, 0, (3.0,)), (1, -1, 0, (60.0,)), (3, 0, 1, (-1.5, 1.5, -1.0, 1.0, -2.5, 0.5))]       # MinDist, MaxDist, BoundingBox
EIGHT = MODS + [(6, 0, 0, ()), (1, 2, 0, (20.0,)), (2, 0, 0, (0.01,)), (3, 0, 0, (-70, 70, -70, 70, -5, 30)), (1, 0, 0, (65.0,))]
CUTS = icp.ChainCuts(tuple(MODS), tuple(MODS), len(MODS))


def filters(mods):
    arr = (_lib.PointFilter * len(mods))()
    for a, (t, d, f, v) in zip(arr, mods):
        a.type, a.dim, a.flag = t, d, f
        for i, x in enumerate(v):
            a.v[i] = x
    return arr


def config(profile):
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.min_diff_rot, cfg.min_diff_trans = 1e-5, 1e-4          # bench.py's
    cfg.profile_kernels = int(profile)
    return cfg


def timed(step, warmup=None):
    for _ in range(args.warmup if warmup is None else warmup):
        step()
    wall, stats = [], []
    for _ in range(args.calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        st = step()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        stats.append(st)
    return wall, stats


def report(name, wall, extra):
    print(json.dumps(dict(figure=name, calls=args.calls, wall_ms_median=round(float(np.median(wall)), 4), wall_ms_min=round(float(np.min(wall)), 4),
                          wall_ms_p90=round(float(np.percentile(wall, 90)), 4), **extra)), flush=True)


def compute_routes(profile):
    with icp.IcpHandle(config(profile)) as h, icp.IcpHandle(config(profile)) as hc:
        hc.set_chain_cuts(CUTS)
        fl = filters(MODS)

        def with_cuts():
            return hc.compute(d_rd, d_ref, T_init, 1.0, 10, 1.0, seed=0)[1]

        def sequential():
            a = h.apply_point_filters(fl, d_rd)
            b = h.apply_point_filters(fl, d_ref)
            return h.compute(a, b, T_init, 1.0, 10, 1.0, seed=0)[1]

        def plain():
            return h.compute(d_rd, d_ref, T_init, 1.0, 10, 1.0, seed=0)[1]

        kept = (int(h.apply_point_filters(fl, d_rd).shape[0]), int(h.apply_point_filters(fl, d_ref).shape[0]))
        for name, step in (("compute_cuts", with_cuts), ("compute_sequential", sequential), ("compute_plain", plain)):
            wall, stats = timed(step)
            med = lambda f: round(float(np.median([f(s) for s in stats])), 4)
            extra = dict(profile_kernels=int(profile), iterations=int(stats[-1].iterations), t_total_ms=med(lambda s: s.t_total_ms),
                         filters_and_grid_ms=med(lambda s: s.t_reserved[0]), points=dict(reading=len(rd), reference=len(ref)),
                         kept_by_cuts=None if name == "compute_plain" else dict(reading=kept[0], reference=kept[1]))
            if profile:
                extra.update(t_knn_ms=med(lambda s: s.t_knn_ms), t_select_ms=med(lambda s: s.t_select_ms), t_ne_ms=med(lambda s: s.t_ne_ms))
            report(name, wall, extra)


def sections():
    with icp.IcpHandle(config(False)) as h:
        for n, mods in ((1, MODS[:1]), (3, MODS), (8, EIGHT)):
            cuts, fl = icp.ChainCuts(tuple(mods), (), len(mods)), filters(mods)
            kept = int(h.filter_section(cuts, 0, d_rd).shape[0])
            assert kept == int(h.apply_point_filters(fl, d_rd).shape[0])
            # (the outputs are dropped at once: 200 kept 16 MB tensors would time torch's allocator, not the pass)
            fused, _ = timed(lambda: h.filter_section(cuts, 0, d_rd) is None, args.section_warmup)
            seq, _ = timed(lambda: h.apply_point_filters(fl, d_rd) is None, args.section_warmup)
            report("section_%d" % n, fused, dict(modules=n, points=len(rd), kept=kept, sequential_wall_ms_median=round(float(np.median(seq)), 4),
                                                 sequential_wall_ms_min=round(float(np.min(seq)), 4),
                                                 speedup_median=round(float(np.median(seq) / np.median(fused)), 3)))


if args.only in ("all", "compute"):
    compute_routes(False)
    compute_routes(True)
if args.only in ("all", "sections"):
    sections()
