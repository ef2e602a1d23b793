"""Sizes at which the two integer primitives change shape -- the prefix scan (csrc/lsgpu_scan.hip.h, scan_u32) and the stable
radix sort (csrc/lsgpu_sort.hip.h, sort_pairs) -- with what each size reaches, the clouds that make order and identity
visible, and numpy references.  numpy and the sources' text only, no device.  Test infrastructure;
tests/test_primitive_sizes.py and tests/prims_worker.py use it.

The constants the tables depend on are read out of the sources (constants()): a change to one of them fails the CPU test
test_sizes_reach_what_the_tables_claim instead of quietly un-covering a path.

What a size reaches.
  scan of m elements: tiles = ceil(m / kScanTile); one launch (k_scan_write alone) for one tile, three (k_scan_sums,
    k_scan_top, k_scan_write) above; the last tile walks ceil(rest / kScanSub) sub-tiles with elements in them; k_scan_top
    walks the tile sums in chunks of 1024 with a carry: ceil(tiles / 1024) chunks.
  per-point flag scans (cylinder crop, RandomSampling, RemoveNaN, the voxel grids' heads, set_reference's chunk flags):
    m = points.  Block-count scans (k_cut_pass, k_md_pass, k_shadow_pass): m = ceil(points / 256).
  sort of n pairs: ITEMS keys per thread = 4 below 2^19 pairs, 8 from there, 16 from 2^21 (LSGPU_SORT_ITEMS forces one);
    blocks = ceil(n / (256 ITEMS)); k_rs_scan walks a digit's block counts in chunks of 256: ceil(blocks / 256) chunks;
    the last block holds n - (blocks - 1) 256 ITEMS keys, its last wave with a key holds (rest - 1) % 64 + 1 valid lanes in
    its last row.

The clouds.  The fourth component of every point is its index (exact in float up to 2^24), so "the kept points, in order, bits
as given" is cloud[mask] byte for byte.  The mask is imposed through geometry: a point lies well inside or well outside
whatever the filter cuts (a NaN for RemoveNaN; a normal along or across the ray for the shadow pass).  Masks are the ones that
make tile sums extreme (PATTERNS); for the block-count scans the same patterns in units of 256-point blocks, a block holding
0, 1 or 256 kept points.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "laser_slam_amd", "csrc")
F = np.float32


# ------------------------------------------------------------------------------------------------ constants from the sources
def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, start, end):
    """The text from the first match of `start` up to the next match of `end` behind it."""
    a = re.search(start, text)
    assert a, start
    b = re.search(end, text[a.end():])
    assert b, (start, end)
    return text[a.start():a.end() + b.start()]


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, (what, found)
    return found[0]


def constants():
    """-> dict of the constants the tables rest on, each parsed from the place that uses it."""
    scan, sort, icp = _read("lsgpu_scan.hip.h"), _read("lsgpu_sort.hip.h"), _read("lsgpu_icp.hip")
    c = {}
    c["scan_sub"] = int(_one(r"constexpr int kScanSub = (\d+);", scan, "kScanSub"))
    c["scan_tile"] = int(_one(r"constexpr int kScanTile = (\d+) \* kScanSub;", scan, "kScanTile")) * c["scan_sub"]
    top = _body(scan, r"void k_scan_top\(", r"\ntemplate <")
    c["top_chunk"] = int(_one(r"for \(int b0 = 0; b0 < nb; b0 \+= (\d+)\)", top, "k_scan_top's chunk"))
    c["top_threads"] = int(_one(r"__launch_bounds__\((\d+)\) void k_scan_top\(", scan, "k_scan_top's block"))
    scan_u32 = _body(icp, r"\nstatic int scan_u32\(lsgpu_icp\* h, const uint32_t\* in, uint32_t\* out, size_t n, bool inclusive, bool nonzero\) \{", r"\n\}\n")
    c["top_launch"] = int(_one(r"k_scan_top, dim3\(1\), dim3\((\d+)\)", scan_u32, "k_scan_top's launch"))
    c["scan_threads"] = int(_one(r"__launch_bounds__\((\d+)\) void k_scan_write\(", scan, "k_scan_write's block"))
    assert re.search(r"const int nb = \(int\)\(\(n \+ kScanTile - 1\) / kScanTile\);", scan_u32) and "if (nb > 1) {" in scan_u32
    rs = _body(sort, r"void k_rs_scan\(", r"\ntemplate <")
    c["rs_chunk"] = int(_one(r"for \(int b0 = 0; b0 < nblocks; b0 \+= (\d+)\)", rs, "k_rs_scan's chunk"))
    c["rs_threads"] = int(_one(r"__launch_bounds__\((\d+)\) void k_rs_scan\(", sort, "k_rs_scan's block"))
    sp = _body(icp, r"\nstatic int sort_pairs\(lsgpu_icp\* h, int64_t n, int nbits\) \{", r"\n\}\n")
    hi, lo = _one(r"items_env \? items_env : n >= \(1 << (\d+)\) \? 16 : n >= \(1 << (\d+)\) \? 8 : 4;", sp, "sort_pairs' thresholds")
    c["items16_from"], c["items8_from"] = 1 << int(hi), 1 << int(lo)
    assert "(n + 256 * items - 1) / (256 * items)" in sp
    c["sort_threads"] = int(_one(r"__launch_bounds__\((\d+)\) void k_rs_scatter\(", sort, "k_rs_scatter's block"))
    # the 256-point block of the rank passes: the kernels' index, their block size and the launches' grid
    blocks = set()
    for name, kernel in (("lsgpu_chain_cut.hip.h", "k_cut_pass"), ("lsgpu_max_density.hip.h", "k_md_pass"), ("lsgpu_shadow.hip.h", "k_shadow_pass")):
        text = _read(name)
        body = _body(text, r"__launch_bounds__\(\d+\) void %s\(" % kernel, r"\n\}\n")
        blocks.add(int(_one(r"__launch_bounds__\((\d+)\) void %s\(" % kernel, body, kernel)))
        blocks.add(int(_one(r"const int i = \(int\)\(blockIdx\.x \* (\d+)u \+ threadIdx\.x\);", body, kernel + "'s index")))
    blocks.add(int(_one(r"inline int nblk\(int64_t n\) \{ return \(int\)\(\(n \+ 255\) / (\d+)\); \}", icp, "nblk")))
    assert len(blocks) == 1, blocks
    c["rank_block"] = blocks.pop()
    for launch in (r"k_cut_pass<0, false>\), dim3\(nb\), dim3\(256\)", r"k_md_pass<0>\), dim3\(nb\), dim3\(256\)", r"k_shadow_pass<0, false>\), dim3\(nb\), dim3\(256\)"):
        assert re.search(launch, icp), launch
    assert len(re.findall(r"const int nb = nblk\(n\);", icp)) >= 3
    return c


# the constants as they are today: the tables below are written with them, test_sizes_reach_what_the_tables_claim compares
SCAN_SUB, SCAN_TILE, TOP_CHUNK, RS_CHUNK, RANK_BLOCK = 1024, 4096, 1024, 256, 256
ITEMS8_FROM, ITEMS16_FROM = 1 << 19, 1 << 21


def scan_shape(m, c=None):
    """What a scan of m elements reaches -> dict(launches, tiles, subs: sub-tiles of the last tile with elements, rest: the
    elements of the last sub-tile, chunks: of k_scan_top (0: not launched), tail: tiles in its last chunk)"""
    c = c or dict(scan_sub=SCAN_SUB, scan_tile=SCAN_TILE, top_chunk=TOP_CHUNK)
    tiles = -(-m // c["scan_tile"])
    last = m - (tiles - 1) * c["scan_tile"]
    subs = -(-last // c["scan_sub"])
    chunks = 0 if tiles == 1 else -(-tiles // c["top_chunk"])
    return dict(launches=1 if tiles == 1 else 3, tiles=tiles, subs=subs, rest=last - (subs - 1) * c["scan_sub"], chunks=chunks,
                tail=0 if chunks == 0 else tiles - (chunks - 1) * c["top_chunk"])


def sort_items(n, c=None):
    c = c or dict(items8_from=ITEMS8_FROM, items16_from=ITEMS16_FROM)
    return 16 if n >= c["items16_from"] else 8 if n >= c["items8_from"] else 4


def sort_shape(n, items=None, c=None):
    """What a sort of n pairs reaches -> dict(items, blocks, chunks: of k_rs_scan, rest: keys of the last block, lanes: valid
    lanes of the last row with a key)"""
    items = items or sort_items(n, c)
    per = 256 * items
    blocks = -(-n // per)
    rest = n - (blocks - 1) * per
    return dict(items=items, blocks=blocks, chunks=-(-blocks // (c or {}).get("rs_chunk", RS_CHUNK)), rest=rest, lanes=(rest - 1) % 64 + 1)


# points -> (launches, tiles, sub-tiles of the last tile, chunks of k_scan_top, tiles in its last chunk, what the size is there for)
FLAG_SIZES = {
    1: (1, 1, 1, 0, 0, "one element: the scalar tail of scan_load4"),
    3: (1, 1, 1, 0, 0, "less than one dwordx4"),
    1023: (1, 1, 1, 0, 0, "one short of a sub-tile: the last thread's load is partial"),
    1024: (1, 1, 1, 0, 0, "exactly one sub-tile"),
    1025: (1, 1, 2, 0, 0, "the carry into a second sub-tile"),
    4095: (1, 1, 4, 0, 0, "one short of a tile"),
    4096: (1, 1, 4, 0, 0, "exactly one tile: the last size with one launch"),
    4097: (3, 2, 1, 1, 2, "the first size with three launches; the second tile holds one element"),
    8192: (3, 2, 4, 1, 2, "two full tiles"),
    8193: (3, 3, 1, 1, 3, "three tiles"),
    12289: (3, 4, 1, 1, 4, "four tiles: every wave of k_scan_top's first row of lanes"),
    4194304: (3, 1024, 4, 1, 1024, "the last size with a single chunk of k_scan_top, full"),
    4194305: (3, 1025, 1, 2, 1, "k_scan_top's second chunk: one tile behind the carry"),
    4198401: (3, 1026, 1, 2, 2, "two tiles in the second chunk"),
}
# points -> (blocks, points of the last block, launches, tiles, sub-tiles of the last tile, what for)
BLOCK_SIZES = {
    1048576: (4096, 256, 1, 1, 4, "4096 blocks: one full tile, the last size with one launch"),
    1048577: (4097, 1, 3, 2, 1, "4097 blocks, the last with one point: the first size with three launches"),
    1048832: (4097, 256, 3, 2, 1, "4097 full blocks"),
    1310721: (5121, 1, 3, 2, 2, "5121 blocks: second tile, second sub-tile begun"),
    2097153: (8193, 1, 3, 3, 1, "three tiles"),
}
# pairs -> (keys per thread, blocks, chunks of k_rs_scan, what for)
SORT_SIZES = {
    262144: (4, 256, 1, "ITEMS 4, the last size with one chunk of k_rs_scan"),
    262145: (4, 257, 2, "ITEMS 4, 257 blocks: k_rs_scan's second chunk, one key in the last block"),
    524287: (4, 512, 2, "the last size with ITEMS 4: a last block one key short"),
    524288: (8, 256, 1, "the first size with ITEMS 8"),
    524289: (8, 257, 2, "ITEMS 8, 257 blocks"),
    2097151: (8, 1024, 4, "the last size with ITEMS 8"),
    2097152: (16, 512, 2, "the first size with ITEMS 16"),
    2097153: (16, 513, 3, "ITEMS 16, 513 blocks, one key in the last"),
}
FORCED_ITEMS = (4, 8, 16)
CHUNK_SCAN_REFERENCE, CHUNK_SCAN_QUERIES = 4194305, 4097    # set_reference's inclusive scan of chunk flags: second chunk


def forced_sizes(items):
    """The worker's sizes under LSGPU_SORT_ITEMS=items, K = 256 items keys per block"""
    k = 256 * items
    return [1, 63, 64, 65, 255, 256, 257, k - 1, k, k + 1, 2 * k + 1] + ([1048577] if items == 16 else [])


# ------------------------------------------------------------------------------------------------ masks
PATTERNS = ("all", "none", "first", "last", "tile_edges", "alternate_tiles", "half")


def mask(m, pattern, tile=SCAN_TILE, seed=0):
    """Which of m scan elements are kept -> bool (m,)"""
    i = np.arange(m)
    if pattern == "all":
        return np.ones(m, bool)
    if pattern == "none":
        return np.zeros(m, bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == m - 1
    if pattern == "tile_edges":
        return (i % tile == 0) | (i % tile == tile - 1)
    if pattern == "alternate_tiles":
        return (i // tile) % 2 == 0
    if pattern == "half":
        return np.random.default_rng(seed * 104729 + m).random(m) < 0.5
    raise KeyError(pattern)


def mask_count(m, pattern, tile=SCAN_TILE):
    """How many elements mask() keeps, by the pattern's definition (None: left to chance)"""
    full, rest = divmod(m, tile)
    return {"all": m, "none": 0, "first": 1, "last": 1, "tile_edges": 2 * full + (1 if rest else 0),
            "alternate_tiles": ((full + 1) // 2) * tile + (rest if full % 2 == 0 else 0), "half": None}[pattern]


def keeps_part(m, pattern, tile=SCAN_TILE):
    """Does the pattern, laid over m elements, claim that some are kept and some are not?"""
    if pattern in ("all", "none") or m < 2:
        return False
    if pattern == "alternate_tiles":
        return m > tile
    if pattern == "tile_edges":
        return m > 2
    return True


def block_mask(n, pattern, block=RANK_BLOCK, tile=SCAN_TILE, seed=0):
    """Which of n points are kept when the pattern is laid over the 256-point blocks -> (bool (n,), kept per block).
    all / alternate_tiles: a chosen block keeps all its points; first / last: the cloud's first / last point alone;
    tile_edges: a chosen block keeps one point, at a place that moves with the block; half: a block keeps none, one or all."""
    nb = -(-n // block)
    size = np.minimum(block, n - np.arange(nb) * block)
    if pattern == "half":
        per = np.random.default_rng(seed * 104729 + n).choice([0, 1, block], nb)
    else:
        chosen = mask(nb, pattern, tile, seed)
        per = np.where(chosen, 1 if pattern in ("first", "last", "tile_edges") else block, 0)
    keep = np.repeat(per == block, block)[:n]
    one = np.flatnonzero(per == 1)
    at = (one * 37) % block
    if pattern == "first":
        at[:] = 0
    if pattern == "last":
        at[:] = size[one] - 1
    keep[one * block + np.minimum(at, size[one] - 1)] = True
    counts = np.add.reduceat(keep.astype(np.int64), np.arange(nb) * block)
    assert set(np.unique(counts).tolist()) <= {0, 1, block} | set(size[-1:].tolist())
    return keep, counts


# ------------------------------------------------------------------------------------------------ clouds
def two_state_cloud(keep, kept_xyz, dropped_xyz):
    """A point per mask entry: kept_xyz or dropped_xyz, x moved by a multiple of 1/8 below 1 that changes with the index
    (exact), the index in the fourth component."""
    n = len(keep)
    assert n <= 1 << 24
    i = np.arange(n)
    p = np.empty((n, 4), F)
    p[:, :3] = np.where(keep[:, None], np.asarray(kept_xyz, F), np.asarray(dropped_xyz, F))
    p[:, 0] += (i % 8).astype(F) * F(0.125)
    p[:, 3] = i.astype(F)
    return p


CYLINDER = dict(center=(0.5, -0.25, 1.0), radius_m=10.0, height_m=8.0)


def cylinder_cloud(keep):
    """Inside: at most 3.9 m from the axis and 0.5 m from the middle; outside: 59 m from the axis"""
    return two_state_cloud(keep, (2.0, 3.0, 1.5), (60.0, 3.0, 1.5))


def cylinder_mask(p, remove_inside=False):
    """applyCylindricalFilter restated (laser_slam_ros common.hpp:194-223): float differences, double squares"""
    c = np.asarray(CYLINDER["center"], F)
    dx, dy = (p[:, 0] - c[0]).astype(np.float64), (p[:, 1] - c[1]).astype(np.float64)
    dz = np.abs(p[:, 2] - c[2]).astype(np.float64)
    r2, rr, hh = dx * dx + dy * dy, CYLINDER["radius_m"] ** 2, CYLINDER["height_m"] / 2.0
    return ((r2 >= rr) | (dz >= hh)) if remove_inside else ((r2 <= rr) & (dz <= hh))


def cut_cloud(keep):
    """For the cut lists `eight`, `sampling_middle` and `sampling_first` of tests/test_chain_cuts.py.  Kept: 11.2 to 12 m
    out, x 10 to 10.9, y 5, z 0.5 -- inside every MaxDist and the keeping box, outside every MinDist and the removing box.
    Dropped: less than 1.5 m out -- short of MinDist 3 and MinDist 5, inside the removing box."""
    return two_state_cloud(keep, (10.0, 5.0, 0.5), (0.5, 0.5, 0.1))


def nan_cloud(keep):
    p = two_state_cloud(keep, (10.0, 5.0, 0.5), (10.0, 5.0, 0.5))
    p[~keep, 0] = np.nan
    return p


def shadow_cloud(keep, seed=0):
    """pattern_cloud of tests/test_shadow_filter.py for a given mask: a kept point's normal lies along its ray (value 1 up
    to rounding), a dropped point's across it (value 0 up to rounding); eps 0.1 separates them whatever the rounding."""
    n = len(keep)
    rng = np.random.default_rng(seed * 7919 + n)
    p = np.empty((n, 4), F)
    p[:, :3] = rng.uniform(1, 20, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    p[:, 3] = np.arange(n, dtype=F)
    along = p[:, :3].astype(np.float64)
    across = np.cross(along, np.array([0.3, -0.5, 0.8]))
    v = np.where(keep[:, None], along, across)
    v = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    return p, v


def uniform_cloud(n, seed=0):
    """n points uniform in a cube with about eight points per unit cell, 0.05 clear of its faces; the index in the fourth
    component -> (cloud, the cube's side)"""
    side = max(2.0, round(float(np.cbrt(n / 8.0)), 3))
    p = np.empty((n, 4), F)
    p[:, :3] = np.random.default_rng(seed * 15485863 + n).uniform(0.05, side - 0.05, (n, 3))
    p[:, 3] = np.arange(n, dtype=F)
    return p, side


def voxel_leaves(side):
    """-> (the leaf with about eight points per voxel, the leaf with 4 x 4 x 4 voxels in all)"""
    return F(1.0), F(side / 4.0)


# the max-density cloud: half the blocks of 256 points lie in a cube of 1 point per unit volume, the other half in a cube of
# 8 per unit volume next to it.  With knn 10 the density descriptor is knn / ((4/3) pi r^3), r the largest distance of a
# neighbour from the neighbourhood's mean: over the whole cloud the host twin gives the percentiles 10 / 25 / 75 / 90 as
# 0.75 / 1.07 / 8.5 / 12.4, at 131 073 and at 400 001 points alike.  MAX_DENSITY lies between the two cubes: about half the
# points are dense, and a dense point is kept with probability MAX_DENSITY / density, about a third.
MAX_DENSITY, MAX_DENSITY_KNN = 3.0, 10


def density_cloud(n, seed=0):
    rng = np.random.default_rng(seed * 32452843 + n)
    nb = -(-n // RANK_BLOCK)
    tight = np.repeat(rng.random(nb) < 0.5, RANK_BLOCK)[:n]
    side = float(np.cbrt(max(1, n - int(tight.sum()))))
    side_t = float(np.cbrt(max(1, int(tight.sum())) / 8.0))
    p = np.empty((n, 4), F)
    p[:, :3] = rng.uniform(0.0, 1.0, (n, 3)) * np.where(tight, side_t, side)[:, None]
    p[tight, 0] += side + 10.0
    p[:, 3] = np.arange(n, dtype=F)
    return p


def max_density_model(dens, max_density, draws):
    """csrc/lsgpu_density.h restated in float32: is_dense, keeps with last / sat, one draw per dense point in order.
    dens (n,) float32; draws(k) -> the first k draws of the stream -> (keep (n,), dense (n,))"""
    dens = np.asarray(dens, F)
    md = F(max_density)
    with np.errstate(invalid="ignore", divide="ignore"):
        dense = dens > md                                           # is_dense: a NaN density is not dense
        num = dens[~np.isnan(dens)]
        last = num.max() if len(num) else F(0)
        sat = F(0 if (len(num) == len(dens) and len(num) and num.min() == last) else 1)
        accept = md / dens[dense]
        assert accept.dtype == F
        accept = np.where(dens[dense] == last, accept * sat, accept)
    keep = np.ones(len(dens), bool)
    keep[dense] = np.asarray(draws(int(dense.sum())), F) < accept
    return keep, dense


# ------------------------------------------------------------------------------------------------ nearest neighbours
def centred(ref, mean):
    c = ref.copy()
    c[:, :3] = ref[:, :3] - np.asarray(mean, F)
    return c


def mean_frame_T(mean):
    """The column-major transform that takes a query into the handle's frame: the identity, the reference mean taken off"""
    T = np.eye(4, dtype=F)
    T[:3, 3] = -np.asarray(mean, F)
    return np.ascontiguousarray(T.T).reshape(16)


def distance_as_defined(q, ref_c, ids):
    """_check_nn's arithmetic (tests/test_gpu_parity.py): fma(dz, dz, fma(dy, dy, dx * dx)) in float32, the differences in
    float32"""
    diff = q[:, :3] - ref_c[ids, :3]
    dx, dy, dz = (diff[:, k].astype(F) for k in range(3))
    dd = (dx * dx).astype(F)
    dd = (dy.astype(np.float64) * dy + dd).astype(F)
    return (dz.astype(np.float64) * dz + dd).astype(F)


def check_knn(oracle, brute, ref, mean, query, ids, d2, sample=256, seed=0):
    """ids / d2 of handle.knn(query, mean_frame_T(mean)) against the definition: every id in range and every d2 the bits of
    the distance to ref[ids] (the bar of _check_nn); for `sample` queries (all, if there are no more) the exact nearest
    neighbour of tests/cpp/knn_brute.c -- the same distance bits, and the same point or one exactly as far.
    -> list of failures in words"""
    f = []
    ref_c = centred(ref, mean)
    q = oracle.transform_points(mean_frame_T(mean), query)
    if not ((ids >= 0) & (ids < len(ref))).all():
        return ["an id out of range: %r" % ids[(ids < 0) | (ids >= len(ref))][:5].tolist()]
    dd = distance_as_defined(q, ref_c, ids)
    bad = np.flatnonzero(dd.view(np.uint32) != d2.view(np.uint32))
    if len(bad):
        f.append("d2 is not the distance to ref[ids] at queries %r" % bad[:5].tolist())
    pick = np.arange(len(q)) if len(q) <= sample else np.sort(np.random.default_rng(seed).choice(len(q), sample, replace=False))
    bi, bd = brute(ref_c, q[pick], 1)
    far = np.flatnonzero(bd[:, 0].view(np.uint32) != d2[pick].view(np.uint32))
    if len(far):
        f.append("not the nearest neighbour at queries %r" % pick[far][:5].tolist())
    return f


# ------------------------------------------------------------------------------------------------ device checks the worker shares
def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pcl_voxel_check(oracle, h, cloud, side, full=True):
    """filter_voxel_grid against oracle.voxel_grid with both leaves, bit for bit -> failures in words"""
    f = []
    fine, coarse = voxel_leaves(side)
    for leaf, name in ((fine, "fine"), (coarse, "coarse")):
        want = oracle.voxel_grid(cloud, [leaf] * 3, 1)
        if name == "coarse" and full and len(want) != 64:
            f.append("the coarse leaf gives %d voxels on the CPU, not 64" % len(want))
        if name == "fine" and full and not 0.05 * len(cloud) < len(want) < 0.5 * len(cloud):
            f.append("the fine leaf gives %d voxels for %d points on the CPU" % (len(want), len(cloud)))
        got = np.ascontiguousarray(h.filter_voxel_grid(cloud, leaf, 1))
        if not same(got, want):
            f.append("filter_voxel_grid, %s leaf: %d voxels for the oracle's %d, or other bits" % (name, len(got), len(want)))
    return f


def chain_voxel_check(h, cloud, side):
    """apply_point_filters with VoxelGridDataPointsFilter (fine leaf, centroids) against ref_voxel_grid of
    tests/test_voxel_grid_filter.py, bit for bit -> failures in words"""
    from laser_slam_amd import _lib
    from test_voxel_grid_filter import _chain, _spec, ref_voxel_grid
    leaf = float(voxel_leaves(side)[0])
    want = ref_voxel_grid(cloud, (leaf, leaf, leaf), 1)[0]
    got = np.ascontiguousarray(h.apply_point_filters(_chain(_lib, [_spec((leaf, leaf, leaf))]), cloud))
    return [] if same(got, want) else ["VoxelGridDataPointsFilter: %d voxels for the restatement's %d, or other bits" % (len(got), len(want))]


def knn_check(oracle, brute, h, ref, query, sample=256):
    """set_reference(ref) and knn(query) -> failures in words (check_knn)"""
    h.set_reference(ref, None)
    mean = h.reference_mean()
    ids, d2 = h.knn(query, mean_frame_T(mean))
    return check_knn(oracle, brute, ref, mean, query, ids, d2, sample)
