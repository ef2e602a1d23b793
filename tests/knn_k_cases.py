"""Cases of tests/test_knn_k_edges.py: the references and query batches that drive the k-nearest search
(csrc/lsgpu_knn_k.hip.h: k_knnk_seed / k_knnk_tile / k_knnk_fallback<K, MAXD>, k_knnk_unpermute) where the scan pairs of the
other tests do not -- exact ties, queries far outside the reference, lists a maxDist leaves partly empty, a level-0 cell with
more than 64 chunks, query counts at the edges of a wave and a block, references of k and k + 1 points -- and the checks the
device's answers are held to.  numpy and the sources' text only, no device.  Test infrastructure.

The constants the cases rest on are read out of the sources (constants()): a change to one of them fails the CPU test
test_constants_are_what_the_cases_were_built_for instead of quietly emptying a case.

Frames.  A handle centres its reference on the float mean of the double coordinate sums and searches in that frame; every
builder here takes that mean (the handle's on the device, predict_geometry's on the CPU: they may differ in the last bit,
which no self-check depends on) and returns queries in the mean frame, to be searched with T = None.

Which path a query takes.  k_knnk_tile hands a query to k_knnk_fallback iff R = sqrt(ub) (1 + 1e-5) + 1e-7 + kFineSlack hf
exceeds kKnnKRCap, ub being the seed's bound cut to maxDist^2.  ub is never below the true k-th distance, so a query whose
k-th distance (or maxDist, if that is smaller) is above kKnnKRCap goes to the fallback NECESSARILY; one whose k-th distance
is well below may still go there on a poor seed.  `necessarily_fallback` is the first class.
"""
import os
import re

import numpy as np

from laser_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------------------------------------ constants from the sources
def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, (what, found)
    return found[0]


def constants():
    """-> dict of the constants the cases rest on, each parsed from the place that defines or uses it."""
    knnk = _read("laser_slam_amd", "csrc", "lsgpu_knn_k.hip.h")
    common = _read("laser_slam_amd", "csrc", "lsgpu_common.hip.h")
    icp = _read("laser_slam_amd", "csrc", "lsgpu_icp.hip")
    api = _read("include", "lsgpu_icp.h")
    make = _read("laser_slam_amd", "csrc", "Makefile")
    c = {}
    c["r_cap"] = float(_one(r"constexpr float kKnnKRCap = ([0-9.]+)f;", knnk, "kKnnKRCap"))
    assert re.search(r"a\.r_cap = kKnnKRCap;", icp)                                 # ... and it is what the launches are handed
    assert re.search(r"const bool wide = valid && !\(R <= a\.r_cap\);", knnk)
    c["chunk_max"] = int(_one(r"#define LSGPU_CHUNK_MAX (\d+)", common, "LSGPU_CHUNK_MAX"))
    assert re.search(r"constexpr int kChunkMax = LSGPU_CHUNK_MAX;", common) and "LSGPU_CHUNK_MAX" not in make
    c["knn_max"] = int(_one(r"#define LSGPU_MATCHER_KNN_MAX (\d+)", api, "LSGPU_MATCHER_KNN_MAX"))
    assert re.search(r"constexpr int kKnnKMax = LSGPU_MATCHER_KNN_MAX;", knnk)
    # one set of kernels per k = 1 .. kKnnKMax, each with maxDist off and on
    assert "= {launch_knn_k<(int)I + 1>...};" in icp and "std::make_index_sequence<kKnnKMax>{}" in icp
    assert "launch_knn_k_<K, true>(h, a, seed)" in icp and "launch_knn_k_<K, false>(h, a, seed)" in icp
    c["fine_slack"] = float(_one(r"constexpr float kFineSlack = ([0-9.]+)f;", common, "kFineSlack"))
    # queries per wave of the tile, per block of the seed, pairs per block of the unpermute; chunks per round of a cell
    c["tile_wave"] = int(_one(r"__launch_bounds__\((\d+)\) void k_knnk_tile\(", knnk, "k_knnk_tile's block"))
    assert re.search(r"const int j = blockIdx\.x \* %d \+ lane;" % c["tile_wave"], knnk)
    c["seed_block"] = int(_one(r"__launch_bounds__\((\d+)\) void k_knnk_seed\(", knnk, "k_knnk_seed's block"))
    assert re.search(r"const int j = blockIdx\.x \* %d \+ threadIdx\.x;" % c["seed_block"], knnk)
    c["unpermute_block"] = int(_one(r"__launch_bounds__\((\d+)\) void k_knnk_unpermute\(", knnk, "k_knnk_unpermute's block"))
    assert re.search(r"const int p = blockIdx\.x \* %d \+ threadIdx\.x;" % c["unpermute_block"], knnk)
    rounds = re.findall(r"for \(uint32_t base = ccs; base < cce; base \+= (\d+)\)", knnk)
    assert len(rounds) == 2 and len(set(rounds)) == 1, rounds                        # the tile's and the fallback's
    c["cell_round"] = int(rounds[0])
    return c


# the constants as they are today: the cases below are written with them
R_CAP, CHUNK_MAX, KNN_MAX, TILE_WAVE, SEED_BLOCK, UNPERMUTE_BLOCK, CELL_ROUND = 1.0, 64, 8, 64, 256, 256, 64
KS = tuple(range(1, KNN_MAX + 1))
MAX_DIST_NEAR, MAX_DIST_WIDE = 0.5, 3.25             # 3.25^2 = 10.5625, both exact in float: above kKnnKRCap^2
MAX_DISTS = (None, MAX_DIST_NEAR, MAX_DIST_WIDE)


def sq(v):
    return F(F(v) * F(v))                                            # one float multiply, as matcher_max_d2


def mean_of(ref):
    """The float mean of the double coordinate sums (numpy's order of additions; the device's may differ in the last bit)."""
    return (np.ascontiguousarray(ref, F)[:, :3].astype(np.float64).sum(0) / float(len(ref))).astype(F)


def centred(ref, mean):
    c = np.ascontiguousarray(ref, F).copy()
    c[:, :3] = c[:, :3] - np.asarray(mean, F)
    return c


def points(xyz):
    p = np.ones((len(xyz), 4), F)
    p[:, :3] = np.asarray(xyz, F)
    return p


def necessarily_fallback(bd2_k, max_dist=None):
    """Queries the tile cannot serve: the search bound, at least the exact k-th distance bd2_k and at most maxDist^2,
    is above kKnnKRCap^2 (+inf, a list the maxDist leaves partly empty, included)."""
    d = np.asarray(bd2_k, F)
    if max_dist:
        d = np.minimum(d, sq(max_dist))
    return d > F(R_CAP * R_CAP)


# ------------------------------------------------------------------------------------------------ the checks
def check_tie_sets(ids, d2, bids, bd2):
    """The rule _check_knn_k leaves open.  _check_knn_k lets the device name another point than the brute force wherever a
    row holds two equal distances; but the two orders -- (d2, Morton-sorted index) on the device, (d2, input index) in the
    brute force -- only permute points WITHIN a distance value, and only the last value of a full list is cut short.  So:
    for every distance value strictly below a row's last valid distance the set of device ids at that value equals the brute
    force's set, and in a row with an invalid entry (the list holds everything within maxDist) at the last value too."""
    assert np.array_equal(d2, bd2)
    k = d2.shape[1]
    valid = np.isfinite(d2)
    nvalid = valid.sum(1)
    last = np.where(nvalid > 0, d2[np.arange(len(d2)), np.maximum(nvalid - 1, 0)], F(-1))
    whole = nvalid < k                                               # nothing was cut off this row but by maxDist
    held = valid & ((d2 < last[:, None]) | whole[:, None])
    dev = np.take_along_axis(ids, np.lexsort((ids, d2), axis=1), axis=1)       # within a value: ascending id
    bru = np.take_along_axis(bids, np.lexsort((bids, bd2), axis=1), axis=1)
    bad = np.flatnonzero(((dev != bru) & held).any(1))
    assert bad.size == 0, (bad[:5], ids[bad[:3]], bids[bad[:3]], d2[bad[:3]])
    return int(held.sum())


def tie_share(d2_wide, k):
    """Share of rows whose k-th and (k+1)-th exact distances are bit-equal (d2_wide: at least k + 1 columns)"""
    return float((d2_wide[:, k - 1].view(np.uint32) == d2_wide[:, k].view(np.uint32)).mean())


# ------------------------------------------------------------------------------------------------ lattice
LATTICE_N, LATTICE_H = 8, 0.5                        # i, j, k in -8..8, 0.5 m apart: 17^3 = 4913 points, every sum exactly 0
CELL, FACE, EDGE, NODE, OUT_ON, OUT_OFF = range(6)
KIND_NAMES = ("cell centre", "face centre", "edge midpoint", "lattice point", "outside, on an axis line", "outside, off it")
# kind -> ((distance, multiplicity), ...) of the nearest points, in order (all exact in float)
LATTICE_TIES = {CELL: ((0.1875, 8),), FACE: ((0.125, 4), (0.375, 8)), EDGE: ((0.0625, 2), (0.3125, 8)),
                NODE: ((0.0, 1), (0.25, 6))}              # (then twelve at 0.5: the 8-th and the 9-th are tied as well)
OUTSIDE = (2.0, 20.0)                                # [m] beyond a face; then d, sqrt(d^2 + 0.25) x 4, ... or 4 x sqrt(d^2 + 0.125)


def lattice(copies=1, n=LATTICE_N):
    """The points 0.5 (i, j, k), i, j, k in -n..n, `copies` times over (copy c of point i is point i + c (2n + 1)^3)"""
    g = np.arange(-n, n + 1, dtype=np.float64) * LATTICE_H
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return points(np.concatenate([xyz] * copies))


def sorted_order(ref, h0=0.125, fine=5):
    """The order set_reference gives a centred reference (k_ref_keys and sort_pairs restated: the Morton key of the
    coordinates counted in steps of h0 / 2^fine from the box's minimum, a stable sort) -> input index by sorted position.
    For clouds whose mean is 0 and whose coordinates are exact multiples of the step, as the lattices' are."""
    p = np.ascontiguousarray(ref, F)[:, :3].astype(np.float64)
    c = np.floor((p - p.min(0)) / (h0 / (1 << fine))).astype(np.int64)
    key = np.zeros(len(p), np.int64)
    for b in range(16):
        for a in range(3):
            key |= ((c[:, a] >> b) & 1) << (3 * b + a)
    return np.argsort(key, kind="stable")


def lattice_queries(seed=3, per_kind=100, n=LATTICE_N):
    """-> (queries (n, 4), kind (n,)): per_kind of each of CELL, FACE, EDGE, NODE (FACE / EDGE / NODE interior, so that the
    second shell is complete; CELL with the eight corner cells among them), and 72 outside queries: OUTSIDE metres beyond
    each of the six faces, on the line through a lattice point and off it by half a step (0.25 m) in both other axes."""
    rng = np.random.default_rng(seed)
    h = LATTICE_H
    q, kind = [], []
    cells = rng.integers(-n, n, (per_kind, 3)).astype(np.float64)
    cells[:8] = [[x, y, z] for x in (-n, n - 1) for y in (-n, n - 1) for z in (-n, n - 1)]
    q.append((cells + 0.5) * h)
    kind += [CELL] * per_kind
    for what, halves in ((FACE, 2), (EDGE, 1)):                      # `halves` axes at a half step, the others on the lattice
        p = rng.integers(-n + 1, n, (per_kind, 3)).astype(np.float64)
        for i in range(per_kind):
            axes = [(i + a) % 3 for a in range(halves)]
            p[i, axes] = rng.integers(-n, n, halves) + 0.5
        q.append(p * h)
        kind += [what] * per_kind
    q.append(rng.integers(-n + 1, n, (per_kind, 3)).astype(np.float64) * h)
    kind += [NODE] * per_kind
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for dist in OUTSIDE:
                for off, what in ((0.0, OUT_ON), (0.5, OUT_OFF)):
                    p = (rng.integers(-n + 2, n - 2, (3, 3)) + off) * h
                    p[:, axis] = sign * (n * h + dist)
                    q.append(p)
                    kind += [what] * 3
    q = points(np.concatenate(q))
    assert np.array_equal(q[:, :3].astype(np.float64) * 4, np.round(q[:, :3].astype(np.float64) * 4))   # quarter steps: exact
    return q, np.asarray(kind)


# ------------------------------------------------------------------------------------------------ far queries, partial lists
CLUSTERS = tuple(range(1, KNN_MAX))                  # a cluster of m points for every m = 1 .. 7
CLUSTER_STEP, CLUSTER_QUERY, CLUSTER_CLEAR = 0.1, 0.3, 20.0
LONELY = (-300.0, 200.0, 90.0)
EDGE_V = (3.0, 4.0, 12.0)                            # x 0.25: |v| = 3.25, squares 0.5625 + 1 + 9 = 10.5625, all exact


def cluster_xyz(m):
    """The m points of cluster m in the frame of the reference as given: 80 m up, 40 m apart, 0.1 m steps along x"""
    c = np.array([40.0 * (m - 4), 10.0, 80.0])
    return c + np.outer(np.arange(m), [CLUSTER_STEP, 0.0, 0.0])


def partial_reference(pair):
    """pair["ref"] plus the clusters -> (reference (n, 4), {m: indices of cluster m})"""
    ref = [np.ascontiguousarray(pair["ref"], F)]
    at, n = {}, len(pair["ref"])
    for m in CLUSTERS:
        ref.append(points(cluster_xyz(m)))
        at[m] = np.arange(n, n + m)
        n += m
    return np.concatenate(ref), at


NEAR_RADIUS, NEAR_PER_POINT, NEAR_JITTER = 0.24, 3, 0.003


def dense_spots(ref, radius=NEAR_RADIUS, k=KNN_MAX):
    """The reference points with k points (themselves included) within `radius` -> indices (double arithmetic, in blocks)"""
    p = np.ascontiguousarray(ref, F)[:, :3].astype(np.float64)
    out = []
    for a in range(0, len(p), 512):
        d = np.sqrt(((p[a:a + 512, None, :] - p[None, :, :]) ** 2).sum(2))
        out.append(a + np.flatnonzero(np.partition(d, k - 1, axis=1)[:, k - 1] < radius))
    return np.concatenate(out)


def far_batch(oracle, pair, mean, seed=11):
    """The queries of test_knn_far_and_outside_queries (tests/test_gpu_parity.py: +-300, +-30, +-3 m about the mean and one at
    (1e4, -1e4, 5e3)), pair["rd"] moved by the initial guess, and NEAR_PER_POINT queries within 3 mm of every reference point
    that has eight points within 0.24 m (a 64-azimuth scan is that dense only close to the sensor: the reading alone brings
    some 70 queries with an 8-th distance below 0.25 m) -- shuffled, so that every prefix mixes them"""
    rng = np.random.default_rng(5)
    q = np.ones((3000, 4), F)
    q[:1000, :3] = rng.uniform(-300, 300, (1000, 3))
    q[1000:2000, :3] = rng.uniform(-30, 30, (1000, 3))
    q[2000:, :3] = rng.uniform(-3, 3, (1000, 3))
    q[0, :3] = (1e4, -1e4, 5e3)
    T = synth.colmajor(pair["T_init"]).copy()
    T[12:15] -= np.asarray(mean, F)
    spots = centred(pair["ref"], mean)[np.repeat(dense_spots(pair["ref"]), NEAR_PER_POINT)]
    spots[:, :3] += np.random.default_rng(seed + 1).uniform(-NEAR_JITTER, NEAR_JITTER, (len(spots), 3)).astype(F)
    batch = np.concatenate([q, oracle.transform_points(T, pair["rd"]), spots]).astype(F)
    return np.ascontiguousarray(batch[np.random.default_rng(seed).permutation(len(batch))])


def partial_queries(ref_c, at):
    """In the mean frame: one query 0.3 m from each cluster (beside its first point, across the cluster's line), one with
    nothing in range, and the edge query at exactly 3.25 m from the one-point cluster -> (queries, {name or m: row}).
    The edge query is cluster point + (3, 4, 12) x 0.25 under the first signed permutation whose three float sums are exact
    (a sum that crosses a power of two may round); the caller asserts the distance it ends up at."""
    rows, q = {}, []
    for m in CLUSTERS:
        rows[m] = len(q)
        q.append(ref_c[at[m][0], :3] + F([0.0, CLUSTER_QUERY, 0.0]))
    rows["lonely"] = len(q)
    q.append(F(LONELY))
    p = ref_c[at[1][0], :3]
    edge = None
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
        for signs in range(8):
            v = F([EDGE_V[i] * 0.25 for i in perm]) * F([1 - 2 * ((signs >> b) & 1) for b in range(3)])
            e = (p + v).astype(F)
            if edge is None and np.array_equal((e - p).astype(F), v):
                edge = e
    assert edge is not None
    rows["edge"] = len(q)
    q.append(edge)
    return points(np.asarray(q, F)), rows


# ------------------------------------------------------------------------------------------------ dense cell
DENSE_CELL_SIZE, DENSE_N, DENSE_SIDE, DENSE_BACKGROUND, DENSE_SPAN = 0.5, 6000, 0.2, 2000, 50.0
DENSE_CELL = (61, 43, 52)                            # the level-0 cell the cube is put into, counted from the box's minimum


def dense_reference(seed=9):
    """2 000 background points uniform over 50 m (its box pinned by two corner points) and 6 000 distinct points in a 0.2 m
    cube in the middle of level-0 cell DENSE_CELL of a 0.5 m grid whose origin is the box's minimum
    -> (reference, indices of the cube's points, the cube's lower corner)"""
    rng = np.random.default_rng(seed)
    half = DENSE_SPAN / 2
    bg = rng.uniform(-half, half, (DENSE_BACKGROUND, 3))
    bg[0], bg[1] = -half, half
    lo = -half + DENSE_CELL_SIZE * np.asarray(DENSE_CELL) + (DENSE_CELL_SIZE - DENSE_SIDE) / 2
    cube = np.unique((lo + rng.uniform(0, DENSE_SIDE, (DENSE_N + 500, 3))).astype(F), axis=0)
    cube = cube[rng.permutation(len(cube))[:DENSE_N]]
    assert len(cube) == DENSE_N
    bg = bg[(np.abs(bg - (lo + DENSE_SIDE / 2)) > 11.0).any(1) | (np.arange(len(bg)) < 2)]    # nothing else within 11 m
    ref = np.concatenate([points(bg), points(cube)])
    return ref, np.arange(len(bg), len(ref)), lo


def level0_cells(ref, geom):
    """The level-0 cell of every reference point, by k_ref_keys' arithmetic in float32 (csrc/lsgpu_grid.hip.h: the origin is
    the box's minimum in the mean frame, fine_coord = floor((c - o) / hf) clamped, the cell its upper `bits` bits)
    -> (cells (n, 3) int, every point's distance from the nearest wall of its cell [m])"""
    p = np.ascontiguousarray(ref, F)[:, :3]
    mean, h0, fine, bits = geom["mean"], F(geom["h0"]), geom["fine"], geom["bits"]
    o = (p.min(0) - mean).astype(F)
    hf = F(h0 / F(1 << fine))
    inv_hf = F(F(1.0) / hf)
    t = np.floor((((p - mean).astype(F) - o).astype(F) * inv_hf).astype(F))
    t = np.clip(t, 0, (1 << (bits + fine)) - 1).astype(np.int64)
    at = ((p - mean).astype(np.float64) - o) / float(h0)
    wall = np.minimum(at - np.floor(at), np.ceil(at) - at).min(1) * float(h0)
    return t >> fine, wall


def dense_queries(lo, seed=10):
    """In the frame of the reference as given: 500 inside the cube, 200 at 0.5 m from its surface, 100 at 5 m"""
    rng = np.random.default_rng(seed)
    mid = lo + DENSE_SIDE / 2
    inside = lo + rng.uniform(0, DENSE_SIDE, (500, 3))
    out = []
    for n, dist in ((200, 0.5), (100, 5.0)):                         # from a point of a face, `dist` along its normal
        p = lo + rng.uniform(0, DENSE_SIDE, (n, 3))
        axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
        p[np.arange(n), axis] = mid[axis] + sign * (DENSE_SIDE / 2 + dist)
        out.append(p)
    return points(np.concatenate([inside] + out)), np.repeat([0, 1, 2], [500, 200, 100])


# ------------------------------------------------------------------------------------------------ query counts, tiny references
QUERY_COUNTS = (1, 63, 64, 65, 255, 256, 257)
QUERY_COUNT_KS = (3, 7)


def tiny_reference(nr, seed=0):
    """nr distinct random points within a few metres"""
    rng = np.random.default_rng(1000 * seed + nr)
    return points(rng.uniform(-3, 3, (nr, 3)))


def tiny_queries(seed=1):
    rng = np.random.default_rng(seed)
    return points(np.concatenate([rng.uniform(-4, 4, (150, 3)), rng.uniform(-60, 60, (50, 3))]))
