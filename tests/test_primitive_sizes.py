"""The prefix scan (csrc/lsgpu_scan.hip.h) and the stable radix sort (csrc/lsgpu_sort.hip.h) past their tile and chunk edges,
through the public calls whose output the primitive determines.  tests/prim_cases.py has the sizes, what each reaches, the
clouds and the numpy references; tests/prims_worker.py is the process that runs under a forced LSGPU_SORT_ITEMS.

CPU part (no marker): the size tables against the constants parsed from the sources (kScanSub, kScanTile, k_scan_top's
1024-tile chunk, k_rs_scan's 256-block chunk, sort_pairs' 2^19 and 2^21, the 256-point block of the rank passes), and the
references' self-checks: the masks keep what their definition says, every cloud builder imposes its mask on the CPU
reference of the filter it is for, the max-density model against the host twin, the nearest-neighbour check against the
oracle's k-d tree and against a planted error.

Device part (one handle for the file; everything selected or integer is compared bit for bit):
  flag scans, points = elements (FLAG_SIZES)     filter_cylinder against the numpy mask and oracle.cylinder_filter, seven
      keep patterns; filter_reading against oracle.random_sampling and the draw stream's position; RemoveNaN alone through
      apply_point_filters; device pointers in and out at 4 194 305.
  block-count scans (BLOCK_SIZES)                filter_section with the cut lists eight / sampling_middle / sampling_first
      of tests/test_chain_cuts.py against oracle.apply_point_filters and the draw stream's position, the reference's side of
      `eight`; filter_shadow against the host twin; filter_reference_max_density against the rule of csrc/lsgpu_density.h
      restated in numpy, fed the device's own densities.
  sort by size (SORT_SIZES)                      filter_voxel_grid against oracle.voxel_grid with two leaves;
      VoxelGridDataPointsFilter against ref_voxel_grid; set_reference + knn against the definition of the distance for every
      query and tests/cpp/knn_brute.c for 256 of them; set_reference at 4 194 305 points (the inclusive scan's second chunk).
  sort forced (forced_sizes)                     three child processes, LSGPU_SORT_ITEMS 4, 8, 16.
A worker that dies, reports a HIP error or overruns its limit fails its test and nothing further is started on the device:
the remaining device tests skip, naming it.

The max-density filter runs at all five block-count sizes (its keep-all filter takes 0.03 to 0.07 s there).

Seen on an MI355X: every device test passes; no defect was found in csrc/.  The max-density model puts 50 to 52 % of the
points above the threshold and keeps 38 % of them.  With k_scan_top's chunk carry taken out of a scratch build, the flag
compaction tests fail at 4 194 305 and 4 198 401 points and nowhere else.

Wall time on an MI355X: 63 to 65 s for the file's 131 device tests (two runs).  VoxelGridDataPointsFilter against
ref_voxel_grid (a Python loop over the points, 3.4 us a point: the one reference here that is not seconds-cheap) 7.0 to 7.5 s at each of the three 2 M-point sizes, 1.5 to 1.7 s at the three around 524 288
and 0.7 to 0.8 s at 262 144 / 262 145; the workers 2.3 to 2.7 s (ITEMS 4 and 8) and 6.2 s (16; 0.4 / 0.4 / 4.3 s of it inside the
worker, 3.8 s of that ref_voxel_grid at 1 048 577 points), the rest interpreter start and library load; filter_cylinder with
seven patterns 1.4 to 1.6 s at each of the three 4 M-point sizes, RemoveNaN 0.85 s, filter_reading 0.34 s there; the 4 194 305-
point set_reference 0.9 s; filter_section at most 0.55 s, the shadow pass at most 0.3 s, max density at most 0.4 s,
filter_voxel_grid and set_reference + knn at most 0.4 s per size; about 7 s for the CPU part.
"""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import chain_cuts_cases as cases
import host_loop
import prim_cases as pc
from chain_cuts_cases import RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER_TIMEOUT = 120    # s (tests/test_reading_sizes.py's): interpreter start, library load, the checked sizes
F = np.float32
SEED = 5
CUT_LISTS = ("eight", "sampling_middle", "sampling_first")
SHADOW_PATTERNS = ("all", "last", "half", "none", "blocks_first", "blocks_tile_edges", "blocks_alternate_tiles", "blocks_half")


@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    return host_loop.build_brute(tmp_path_factory.mktemp("knn_brute"))


def section_lists():
    import test_chain_cuts
    return {name: test_chain_cuts.SECTION_LISTS[name] for name in CUT_LISTS}


def empty():
    return np.empty((0, 4), F)


# ------------------------------------------------------------------------------------------------ the tables, on the CPU
def test_sizes_reach_what_the_tables_claim():
    c = pc.constants()
    assert (c["scan_sub"], c["scan_tile"], c["top_chunk"], c["rs_chunk"], c["rank_block"]) == \
        (pc.SCAN_SUB, pc.SCAN_TILE, pc.TOP_CHUNK, pc.RS_CHUNK, pc.RANK_BLOCK)
    assert (c["items8_from"], c["items16_from"]) == (pc.ITEMS8_FROM, pc.ITEMS16_FROM)
    # a chunk is what one block of the kernel takes at a time; a sub-tile one dwordx4 per thread
    assert c["top_chunk"] == c["top_threads"] == c["top_launch"] and c["rs_chunk"] == c["rs_threads"]
    assert c["scan_sub"] == 4 * c["scan_threads"] and c["sort_threads"] == 256
    # the issue's lists
    assert sorted(pc.FLAG_SIZES) == [1, 3, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, 12289, 4194304, 4194305, 4198401]
    assert sorted(pc.BLOCK_SIZES) == [1048576, 1048577, 1048832, 1310721, 2097153]
    assert sorted(pc.SORT_SIZES) == [262144, 262145, 524287, 524288, 524289, 2097151, 2097152, 2097153]
    for n, (launches, tiles, subs, chunks, tail, _why) in pc.FLAG_SIZES.items():
        s = pc.scan_shape(n, c)
        assert (s["launches"], s["tiles"], s["subs"], s["chunks"], s["tail"]) == (launches, tiles, subs, chunks, tail), (n, s)
    shape = {n: pc.scan_shape(n, c) for n in pc.FLAG_SIZES}
    assert shape[1]["rest"] == 1 and shape[3]["rest"] == 3 and shape[1023]["rest"] == 1023 and shape[1025]["rest"] == 1
    assert shape[4096]["launches"] == 1 and shape[4097]["launches"] == 3                      # the threshold between the two
    assert shape[4194304]["chunks"] == 1 and shape[4194304]["tail"] == c["top_chunk"]         # the last single chunk, full
    assert shape[4194305]["chunks"] == 2 and shape[4198401]["tail"] == 2
    for n, (blocks, last, launches, tiles, subs, _why) in pc.BLOCK_SIZES.items():
        assert blocks == -(-n // c["rank_block"]) and last == n - (blocks - 1) * c["rank_block"], n
        s = pc.scan_shape(blocks, c)
        assert (s["launches"], s["tiles"], s["subs"]) == (launches, tiles, subs), (n, s)
        assert s["chunks"] <= 1 and n <= 1 << 24
    assert max(-(-n // c["rank_block"]) for n in (4099, 16384)) <= 64 < c["scan_sub"]         # what the small-size tests reach
    for n, (items, blocks, chunks, _why) in pc.SORT_SIZES.items():
        s = pc.sort_shape(n, None, c)
        assert (s["items"], s["blocks"], s["chunks"]) == (items, blocks, chunks), (n, s)
    sort = {n: pc.sort_shape(n, None, c) for n in pc.SORT_SIZES}
    assert sort[262145]["rest"] == 1 and sort[524287]["rest"] == 1023 and sort[524287]["lanes"] == 63
    assert sort[524289]["rest"] == 1 and sort[2097151]["rest"] == 2047 and sort[2097153]["rest"] == 1
    assert pc.sort_items(c["items8_from"] - 1, c) == 4 and pc.sort_items(c["items16_from"] - 1, c) == 8
    for items in pc.FORCED_ITEMS:
        k = 256 * items
        sizes = pc.forced_sizes(items)
        assert sizes[:11] == [1, 63, 64, 65, 255, 256, 257, k - 1, k, k + 1, 2 * k + 1]
        got = [pc.sort_shape(n, items, c) for n in sizes]
        assert [s["blocks"] for s in got[:11]] == [1] * 9 + [2, 3]
        assert [s["lanes"] for s in got[:7]] == [1, 63, 64, 1, 63, 64, 1] and got[7]["lanes"] == 63 and got[8]["rest"] == k
        assert got[9]["rest"] == 1 and got[10]["rest"] == 1
        if items != 4:      # below 2^19 pairs the library would take 4 by itself: only a forced process reaches these
            assert all(pc.sort_items(n, c) != items for n in sizes)
    big = pc.sort_shape(1048577, 16, c)
    assert pc.forced_sizes(16)[-1] == 1048577 and (big["blocks"], big["chunks"], big["rest"]) == (257, 2, 1)
    s = pc.scan_shape(pc.CHUNK_SCAN_REFERENCE, c)
    assert (s["chunks"], s["tail"]) == (2, 1) and pc.scan_shape(pc.CHUNK_SCAN_QUERIES, c)["launches"] == 3


# ------------------------------------------------------------------------------------------------ the references' self-checks
@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_masks_keep_what_their_definition_says(pattern):
    for m in list(pc.FLAG_SIZES) + [blocks for blocks, *_ in pc.BLOCK_SIZES.values()]:
        k = pc.mask(m, pattern)
        want = pc.mask_count(m, pattern)
        assert pattern == "half" and m < 64 or (0 < k.sum() < m) == pc.keeps_part(m, pattern), (m, pattern)
        if want is not None:
            assert k.sum() == want, (m, pattern)
        else:
            assert m < 64 or 0.3 * m < k.sum() < 0.7 * m, (m, pattern)
        if pattern == "tile_edges" and m > pc.SCAN_TILE + 1:
            assert k[pc.SCAN_TILE - 1] and k[pc.SCAN_TILE] and not k[pc.SCAN_TILE + 1]
        if pattern == "alternate_tiles" and m >= 2 * pc.SCAN_TILE:
            assert k[:pc.SCAN_TILE].all() and not k[pc.SCAN_TILE:2 * pc.SCAN_TILE].any()
    for n in pc.BLOCK_SIZES:
        keep, counts = pc.block_mask(n, pattern)
        last = n - (len(counts) - 1) * pc.RANK_BLOCK
        assert (0 < keep.sum() < n) == pc.keeps_part(len(counts), pattern), (n, pattern)
        assert keep.sum() == counts.sum() and set(np.unique(counts).tolist()) <= {0, 1, pc.RANK_BLOCK, last}
        if pattern == "all":
            assert keep.all()
        elif pattern == "none":
            assert not keep.any()
        elif pattern == "first":
            assert keep[0] and keep.sum() == 1
        elif pattern == "last":
            assert keep[-1] and keep.sum() == 1
        elif pattern == "tile_edges":
            assert keep.sum() == pc.mask_count(len(counts), pattern) and set(np.unique(counts).tolist()) == {0, 1}
        elif pattern == "alternate_tiles":
            assert counts[:pc.SCAN_TILE].min() == pc.RANK_BLOCK
            assert keep.all() if len(counts) == pc.SCAN_TILE else (0 < keep.sum() < n and counts[pc.SCAN_TILE] == 0)
        else:
            assert all(0.25 * len(counts) < (counts == v).sum() for v in (0, 1, pc.RANK_BLOCK)) and 0 < keep.sum() < n


def test_clouds_impose_their_mask_on_the_cpu_references(oracle):
    from laser_slam_amd import icp
    lists = section_lists()
    of = lambda mods: cases.point_filters(mods, cls=oracle.PointFilter)
    for n in (1, 257, 12289):
        for pattern in pc.PATTERNS:
            k = pc.mask(n, pattern)
            p = pc.cylinder_cloud(k)
            assert np.array_equal(p[:, 3], np.arange(n)) and np.array_equal(pc.cylinder_mask(p), k)
            assert np.array_equal(pc.cylinder_mask(p, True), ~k)
            assert oracle.cylinder_filter(p, pc.CYLINDER["center"], pc.CYLINDER["radius_m"], pc.CYLINDER["height_m"], False).tobytes() == p[k].tobytes()
            q = pc.nan_cloud(k)
            got = oracle.apply_point_filters(of([(6, 0, 0, [])]), q)
            assert (empty() if got is None else got).tobytes() == q[k].tobytes()
    n = 1048577
    for pattern in pc.PATTERNS:
        keep, _counts = pc.block_mask(n, pattern)
        p = pc.cut_cloud(keep)
        for name, mods in lists.items():
            got = oracle.apply_point_filters(of(mods), p, seed=SEED)
            got = empty() if got is None else got
            if RS not in mods:
                assert got.tobytes() == p[keep].tobytes(), (pattern, name)
            else:       # what the cuts keep, thinned by the draws: a subsequence of p[keep]
                idx = got[:, 3].astype(np.int64)
                assert keep[idx].all() and np.all(np.diff(idx) > 0) and got.tobytes() == p[idx].tobytes(), (pattern, name)
                if keep.sum() > 1000:
                    assert 0.4 * keep.sum() < len(got) < 0.6 * keep.sum(), (pattern, name)
        if pattern != "none":
            sp, sv = pc.shadow_cloud(keep)
            wp, wn = icp.shadow(sp, sv, 0.1)
            assert pc.same(wp, sp[keep]) and pc.same(wn, sv[keep]), pattern


def test_max_density_model_equals_the_host_twin():
    from laser_slam_amd import icp
    from test_max_density import libc_draws
    n = 20001
    cloud = pc.density_cloud(n)
    nrm, dens = icp.surface_normal(cloud, pc.MAX_DENSITY_KNN, with_densities=True)
    keep, dense = pc.max_density_model(dens, pc.MAX_DENSITY, lambda k: libc_draws(17, 0, k))
    print("dense", dense.mean(), "kept of the dense", keep[dense].mean())
    assert 0.2 <= dense.mean() <= 0.8 and 0.1 <= keep[dense].mean() <= 0.9
    out, out_n, n_dense, d = icp.max_density(cloud, pc.MAX_DENSITY_KNN, pc.MAX_DENSITY, 17)
    assert n_dense == dense.sum() and pc.same(d, dens)
    assert out.tobytes() == cloud[keep].tobytes() and pc.same(out_n, nrm[keep])
    # every density equal (sat 0): everything dense is dropped whatever the draw; a NaN density is kept without a draw, and
    # with one in the cloud sat is 1: the others are drawn for
    flat = np.full(8, 7.0, F)
    k, ds = pc.max_density_model(flat, 3.0, lambda m: np.zeros(m, F))
    assert ds.all() and not k.any()
    flat[3] = np.nan
    k, ds = pc.max_density_model(flat, 3.0, lambda m: np.full(m, 0.9, F))
    assert ds.sum() == 7 and k.sum() == 1 and k[3]
    k, ds = pc.max_density_model(flat, 3.0, lambda m: np.full(m, 0.4, F))      # 0.4 < 3 / 7
    assert ds.sum() == 7 and k.all()


def test_knn_check_accepts_the_kd_tree_and_sees_a_planted_error(oracle, brute):
    ref, side = pc.uniform_cloud(5001)
    query = pc.uniform_cloud(777, seed=1)[0]
    mean = (ref[:, :3].astype(np.float64).sum(0) / len(ref)).astype(F)
    q = oracle.transform_points(pc.mean_frame_T(mean), query)
    assert np.array_equal(q[:, :3], query[:, :3] - mean)
    ids, d2 = oracle.KdTree(pc.centred(ref, mean)).nn(q)
    assert pc.check_knn(oracle, brute, ref, mean, query, ids, d2) == []
    wrong = ids.copy()
    wrong[5] = (wrong[5] + 1) % len(ref)
    assert any("not the distance" in f for f in pc.check_knn(oracle, brute, ref, mean, query, wrong, d2, sample=777))
    far_d2 = pc.distance_as_defined(q, pc.centred(ref, mean), wrong)
    assert any("not the nearest" in f for f in pc.check_knn(oracle, brute, ref, mean, query, wrong, far_d2, sample=777))
    wrong[6] = len(ref)
    assert any("out of range" in f for f in pc.check_knn(oracle, brute, ref, mean, query, wrong, d2))


# ------------------------------------------------------------------------------------------------ the device runs
_STOPPED = None     # why nothing further is started on the device
_POSITIONS = {}


def _device_or_skip():
    if _STOPPED:
        pytest.skip("nothing more on the device after " + _STOPPED)


def _guard(fn, what):
    """Runs fn(); a HIP error stops every later device test of this file."""
    global _STOPPED
    from laser_slam_amd._lib import HIP_ERROR, LsgpuError
    try:
        return fn()
    except LsgpuError as e:
        if e.code == HIP_ERROR:
            _STOPPED = f"a HIP error in {what}"
        raise


@pytest.fixture(scope="module")
def handle():
    from laser_slam_amd import icp
    with icp.IcpHandle() as h:
        yield h


def expected_position(seed, consumed):
    """cases.stream_position() of a library stream seeded with `seed` that has given `consumed` draws (host code only)"""
    from laser_slam_amd import icp
    if (seed, consumed) not in _POSITIONS:
        icp.random_sampling(consumed, 0.5, seed=seed)
        _POSITIONS[(seed, consumed)] = cases.stream_position()
    return _POSITIONS[(seed, consumed)]


@functools.lru_cache(maxsize=2)
def uniform(n):
    cloud, side = pc.uniform_cloud(n)
    cloud.setflags(write=False)
    return cloud, side


# ---- flag compaction
@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.FLAG_SIZES))
def test_cylinder_compaction_at_flag_scan_sizes(n, handle, oracle):
    _device_or_skip()
    cyl = pc.CYLINDER
    t0 = time.perf_counter()
    for pattern in pc.PATTERNS:
        k = pc.mask(n, pattern)
        p = pc.cylinder_cloud(k)
        assert np.array_equal(pc.cylinder_mask(p), k)
        got = _guard(lambda: handle.filter_cylinder(p, cyl["center"], cyl["radius_m"], cyl["height_m"], False), f"filter_cylinder, {n} points")
        assert len(got) == k.sum() and got.tobytes() == p[k].tobytes(), (n, pattern, len(got), int(k.sum()))
        assert oracle.cylinder_filter(p, cyl["center"], cyl["radius_m"], cyl["height_m"], False).tobytes() == p[k].tobytes(), (n, pattern)
        if pattern == "half":       # ... and the complement
            got = _guard(lambda: handle.filter_cylinder(p, cyl["center"], cyl["radius_m"], cyl["height_m"], True), f"filter_cylinder, {n} points")
            assert got.tobytes() == p[~k].tobytes(), (n, pattern)
            assert oracle.cylinder_filter(p, cyl["center"], cyl["radius_m"], cyl["height_m"], True).tobytes() == p[~k].tobytes()
    print("n", n, pc.scan_shape(n), "%.2f s" % (time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.FLAG_SIZES))
def test_random_sampling_compaction_at_flag_scan_sizes(n, handle, oracle):
    _device_or_skip()
    p = pc.nan_cloud(np.ones(n, bool))
    probs = (0.5, 1.0, 0.0) if n in sorted(pc.FLAG_SIZES)[-3:] else (0.5,)
    for prob in probs:
        keep = oracle.random_sampling(n, prob, 7)
        if prob == 0.5:
            assert n < 63 or 0 < len(keep) < n
        if prob == 0.0:
            assert len(keep) == 0
        if prob == 1.0:
            assert len(keep) >= n - 1       # (a draw of exactly 1 is not below 1)
        got = _guard(lambda: handle.filter_reading(p, prob, seed=7), f"filter_reading, {n} points")
        pos = cases.stream_position()
        assert len(got) == len(keep) and got.tobytes() == p[keep].tobytes(), (n, prob, len(got), len(keep))
        assert pos == expected_position(7, n), (n, prob)


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.FLAG_SIZES))
def test_remove_nan_compaction_at_flag_scan_sizes(n, handle):
    _device_or_skip()
    for pattern in pc.PATTERNS:
        k = pc.mask(n, pattern)
        p = pc.nan_cloud(k)
        got = _guard(lambda: handle.apply_point_filters(cases.point_filters([(6, 0, 0, [])]), p), f"RemoveNaN, {n} points")
        assert len(got) == k.sum() and np.ascontiguousarray(got).tobytes() == p[k].tobytes(), (n, pattern, len(got), int(k.sum()))


@pytest.mark.gpu
def test_flag_compaction_on_device_pointers(handle):
    _device_or_skip()
    import torch
    n = 4194305
    assert pc.scan_shape(n)["chunks"] == 2
    cyl = pc.CYLINDER
    k = pc.mask(n, "half")
    p = pc.cylinder_cloud(k)
    d = torch.from_numpy(p).cuda()
    got = _guard(lambda: handle.filter_cylinder(d, cyl["center"], cyl["radius_m"], cyl["height_m"], False), "filter_cylinder on device pointers")
    assert got.is_cuda and got.cpu().numpy().tobytes() == p[k].tobytes()
    assert d.cpu().numpy().tobytes() == p.tobytes()            # the input is only read


# ---- rank passes
@pytest.mark.gpu
@pytest.mark.parametrize("name", CUT_LISTS)
@pytest.mark.parametrize("n", list(pc.BLOCK_SIZES))
def test_filter_section_at_block_count_sizes(n, name, handle, oracle):
    _device_or_skip()
    from laser_slam_amd import icp
    mods = section_lists()[name]
    cuts = cases.chain_cuts(mods)
    prob = cases.PROB if RS in mods else -1.0
    t0 = time.perf_counter()
    for pattern in pc.PATTERNS:
        keep, _counts = pc.block_mask(n, pattern)
        p = pc.cut_cloud(keep)
        want = oracle.apply_point_filters(cases.point_filters(mods, cls=oracle.PointFilter), p, seed=SEED)
        want = empty() if want is None else np.ascontiguousarray(want)
        consumed = 0 if RS not in mods else n if mods[0] == RS else int(keep.sum())   # the points that reach RandomSampling
        if RS not in mods:
            assert want.tobytes() == p[keep].tobytes()
        elif pattern in ("all", "alternate_tiles", "half"):     # the draws thin what the cuts keep
            assert 0 < len(want) < keep.sum()
        assert (0 < keep.sum() < n) == pc.keeps_part(len(_counts), pattern) and (pattern != "all" or keep.all())
        got = _guard(lambda: handle.filter_section(cuts, 0, p, prob=prob, seed=SEED), f"filter_section {name}, {n} points")
        pos = cases.stream_position()
        assert len(got) == len(want) and np.ascontiguousarray(got).tobytes() == want.tobytes(), (n, name, pattern, len(got), len(want))
        assert pos == expected_position(SEED, consumed), (n, name, pattern)
        if name == "eight":                                     # the reference's side of the same modules
            ref_side = _guard(lambda: handle.filter_section(icp.ChainCuts((), cuts.reading, 0), 1, p, prob=0.5, seed=SEED), f"filter_section {name}, {n} points")
            assert np.ascontiguousarray(ref_side).tobytes() == want.tobytes() and cases.stream_position() == expected_position(SEED, 0), (n, pattern)
    print("n", n, name, "%.2f s" % (time.perf_counter() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", SHADOW_PATTERNS)
@pytest.mark.parametrize("n", list(pc.BLOCK_SIZES))
def test_shadow_pass_at_block_count_sizes(n, pattern, handle):
    _device_or_skip()
    from laser_slam_amd import _lib, icp
    if pattern.startswith("blocks_"):
        keep, _counts = pc.block_mask(n, pattern[len("blocks_"):])
        p, v = pc.shadow_cloud(keep)
    else:
        from test_shadow_filter import pattern_cloud
        p, v, keep = pattern_cloud(n, pattern)
        p[:, 3] = np.arange(n, dtype=F)                         # (not read by the module: the point's index)
    if pattern == "none":
        with pytest.raises(_lib.ConvergenceError) as e:
            _guard(lambda: handle.filter_shadow(p, v, 0.1), f"filter_shadow, {n} points")
        assert "left no point" in str(e.value)
        return
    want_p, want_n = icp.shadow(p, v, 0.1)
    assert len(want_p) == keep.sum() and pc.same(want_p, p[keep]) and pc.same(want_n, v[keep]), (n, pattern)
    blocks = -(-n // pc.RANK_BLOCK)
    assert (0 < keep.sum() < n) == pc.keeps_part(blocks, pattern.replace("blocks_", "")) and (pattern != "all" or keep.all())
    got_p, got_n = _guard(lambda: handle.filter_shadow(p, v, 0.1), f"filter_shadow, {n} points")
    assert len(got_p) == len(want_p), (n, pattern, len(got_p), len(want_p))
    assert pc.same(got_p, want_p) and pc.same(got_n, want_n), (n, pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.BLOCK_SIZES))
def test_max_density_at_block_count_sizes(n, handle):
    _device_or_skip()
    from test_max_density import libc_draws
    knn, md, seed = pc.MAX_DENSITY_KNN, pc.MAX_DENSITY, 17
    cloud = pc.density_cloud(n)
    t0 = time.perf_counter()
    nrm, dens = _guard(lambda: handle.filter_reference_normals(cloud, knn, with_densities=True), f"filter_reference_normals, {n} points")
    t1 = time.perf_counter()
    keep, dense = pc.max_density_model(dens, md, lambda k: libc_draws(seed, 0, k))
    print("n", n, "dense", dense.mean(), "kept of the dense", keep[dense].mean(), "keep-all filter %.2f s" % (t1 - t0))
    assert 0.2 <= dense.mean() <= 0.8 and 0.1 <= keep[dense].mean() <= 0.9      # on the model
    t0 = time.perf_counter()
    got_p, got_n, n_dense = _guard(lambda: handle.filter_reference_max_density(cloud, knn, md, seed), f"filter_reference_max_density, {n} points")
    print("max density %.2f s" % (time.perf_counter() - t0))
    pos = cases.stream_position()
    assert n_dense == dense.sum() and len(got_p) == keep.sum(), (n, n_dense, int(dense.sum()), len(got_p), int(keep.sum()))
    assert np.ascontiguousarray(got_p).tobytes() == cloud[keep].tobytes()
    assert pc.same(got_n, nrm[keep])
    assert pos == expected_position(seed, int(dense.sum()))     # one draw per dense point


# ---- the sort, by size
@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.SORT_SIZES))
def test_pcl_voxel_grid_at_sort_sizes(n, handle, oracle):
    _device_or_skip()
    cloud, side = uniform(n)
    f = _guard(lambda: pc.pcl_voxel_check(oracle, handle, cloud, side), f"filter_voxel_grid, {n} points")
    assert not f, (n, pc.sort_shape(n), f)


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.SORT_SIZES))
def test_chain_voxel_grid_at_sort_sizes(n, handle):
    _device_or_skip()
    cloud, side = uniform(n)
    f = _guard(lambda: pc.chain_voxel_check(handle, cloud, side), f"VoxelGridDataPointsFilter, {n} points")
    assert not f, (n, pc.sort_shape(n), f)


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(pc.SORT_SIZES))
def test_set_reference_and_knn_at_sort_sizes(n, handle, oracle, brute):
    _device_or_skip()
    cloud, _side = uniform(n)
    query = pc.uniform_cloud(n, seed=1)[0]
    f = _guard(lambda: pc.knn_check(oracle, brute, handle, cloud, query), f"set_reference + knn, {n} points")
    assert not f, (n, pc.sort_shape(n), f)


@pytest.mark.gpu
def test_set_reference_past_the_inclusive_scans_first_chunk(handle, oracle, brute):
    """4 194 305 reference points: k_scan_top's second chunk under set_reference's inclusive scan of the chunk flags.  Every
    one of the 4 097 queries against the brute-force search."""
    _device_or_skip()
    cloud, side = pc.uniform_cloud(pc.CHUNK_SCAN_REFERENCE)
    query = np.ones((pc.CHUNK_SCAN_QUERIES, 4), F)
    query[:, :3] = np.random.default_rng(3).uniform(0.0, side, (len(query), 3))      # all over the reference's cube
    f = _guard(lambda: pc.knn_check(oracle, brute, handle, cloud, query, sample=len(query)), "set_reference + knn, 4 194 305 points")
    assert not f, f


# ---- the sort, forced
@pytest.mark.gpu
@pytest.mark.timeout(180)
@pytest.mark.parametrize("items", pc.FORCED_ITEMS)
def test_forced_sort_items(items):
    """tests/prims_worker.py with LSGPU_SORT_ITEMS set (and nothing else): one wave, one block, two and three blocks of the
    8- and 16-key instantiations, which the library takes by itself only from 2^19 and 2^21 pairs on."""
    global _STOPPED
    _device_or_skip()
    env = dict(os.environ)
    env["LSGPU_SORT_ITEMS"] = str(items)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "prims_worker.py")]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STOPPED = f"the worker with LSGPU_SORT_ITEMS={items} overran its {WORKER_TIMEOUT} s"
        pytest.fail(_STOPPED)
    res = [json.loads(ln[len("PRIM_RESULT "):]) for ln in p.stdout.splitlines() if ln.startswith("PRIM_RESULT ")]
    done = [json.loads(ln[len("PRIM_DONE "):]) for ln in p.stdout.splitlines() if ln.startswith("PRIM_DONE ")]
    hip = [r for r in res if r.get("code") == 3]
    if hip:
        _STOPPED = f"a HIP error in the worker with LSGPU_SORT_ITEMS={items}, {hip[0]['n']} points"
        pytest.fail(f"{_STOPPED}: {hip[0]}")
    if p.returncode != 0 or len(done) != 1:
        _STOPPED = f"the worker with LSGPU_SORT_ITEMS={items} ended with status {p.returncode}"
        pytest.fail(f"{_STOPPED}\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
    print("worker, ITEMS", items, "%.2f s in the worker, %.2f s in all" % (done[0]["seconds"], time.perf_counter() - t0),
          [(r["n"], round(r.get("seconds", -1.0), 2)) for r in res])
    assert "LSGPU_SORT_ITEMS" not in p.stderr, p.stderr[-1500:]   # (the library says so when it does not take the value)
    assert done[0]["items"] == items and [r["n"] for r in res] == pc.forced_sizes(items) == done[0]["sizes"]
    for r in res:
        assert "error" not in r, r
        assert r["failures"] == [], (items, r["n"], pc.sort_shape(r["n"], items), r["failures"])
