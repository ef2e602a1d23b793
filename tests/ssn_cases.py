"""Sizes and tree shapes of the reference filter's box tree (SamplingSurfaceNormalDataPointsFilter on the device: ssn_device in
csrc/lsgpu_icp.hip, the sort-free upper levels of csrc/lsgpu_ssn_select.hip.h, the segmented-sort levels, k_ssn_tree<B> of
csrc/lsgpu_ssn_tree.hip.h), with what each (n, knn, B) reaches, and the clouds that make the order of ties visible.  numpy
and the sources' text only, no device.  Test infrastructure; tests/test_reference_filter_shapes.py and tests/ssn_worker.py
use it.

The constants the tables depend on are read out of the sources (constants()): a change to one of them fails the CPU test
test_sizes_reach_what_the_tables_claim instead of quietly un-covering a path.

What a size reaches (shape()).  The tree has `levels` levels: the largest child keeps count - count / 2 points, until a box
holds at most knn.  The first `glevels` of them are global passes over the whole cloud, the other `rem` run inside one
workgroup per root, B points at most.  A level goes global while its largest segment holds more than B points (the size
clause) or more than log2(B / 8) levels are left (the depth clause: k_ssn_tree has B / 8 leaf slots).  A global level walks a
segment in blocks of kGsTile positions; k_gs_select runs with 1024 threads at levels 0 to 2 and 256 from level 3 on.  Inside
the workgroup a segment that is finished (count <= knn) before the last level carries over as child 2s; child 2s + 1 is an
empty leaf slot.

The clouds (cloud()), xyz1 float32, seeded by (kind, n):
  smooth     uniform in a 60 x 35 x 8 m box round the origin, every coordinate of an axis distinct: no tie anywhere; the cut
             axis changes with the depth
  quantised  normal draws scaled by (40, 25, 6), rounded, a quarter of that (the `grid` of
             test_device_reference_filter_edge_cases): runs of equal coordinates at the global levels and inside the workgroups
  sheet      quantised with z constant: that axis has range 0 in every root (the presort's P == 0 branch), the cuts alternate
             between the other two
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
    icp, sel, tree, ssn = _read("lsgpu_icp.hip"), _read("lsgpu_ssn_select.hip.h"), _read("lsgpu_ssn_tree.hip.h"), _read("lsgpu_ssn.hip.h")
    dev = _body(icp, r"\nstatic int ssn_device\(lsgpu_icp\* h, const float4\* src, int64_t n, int knn,", r"\n\}\n")
    c = {}
    # the plan: levels, the root size by the cloud's size, the levels a root holds, the two clauses
    assert "for (int64_t c = n; c > knn; c -= c / 2) ++levels;" in dev
    m = _one(r"const int root_auto = n >= (\d+)ll \* (\d+) \? (\d+) : n >= (\d+)ll \* (\d+) \? (\d+) : (\d+);", dev, "root_auto")
    f8, b8, r8, f4, b4, r4, r2 = (int(v) for v in m)
    assert b8 == r8 and b4 == r4
    c["roots"] = (r2, r4, r8)
    c["root_from"] = {r4: f4 * b4, r8: f8 * b8}
    assert "const int root_max = tuning().ssn_root ? tuning().ssn_root : root_auto;" in dev
    c["leaf_floor"] = int(_one(r"while \(\((\d+) << root_levels\) < root_max\) \+\+root_levels;", dev, "root_levels"))
    assert "while (glevels < levels && !(c <= root_max && levels - glevels <= root_levels)) { c -= c / 2; ++glevels; }" in dev
    assert "const bool select_levels = !force_sort_levels && !tuning().ssn_sort_levels && glevels > 0;" in dev
    # the launches of the tree kernel: B / 8 threads each, 1 << glevels workgroups
    launches = re.findall(r"hipLaunchKernelGGL\(k_ssn_tree<(\d+)>, dim3\(1 << glevels\), dim3\((\d+)\),", dev)
    c["tree_threads"] = {int(b): int(t) for b, t in launches}
    assert len(launches) == 3 and "if (root_max == 8192)" in dev and "else if (root_max == 4096)" in dev
    # the sort-free levels
    c["gs_tile"] = int(_one(r"constexpr uint32_t kGsTile = (\d+)u;", sel, "kGsTile"))
    c["gs_cand_cap"] = int(_one(r"constexpr uint32_t kGsCandCap = (\d+)u;", sel, "kGsCandCap"))
    c["gs_part_threads"] = int(_one(r"constexpr int kGsPartThreads = (\d+);", sel, "kGsPartThreads"))
    lvl, wide, narrow = _one(r"k_gs_select, dim3\(ns\), dim3\(L < (\d+) \? (\d+) : (\d+)\)", dev, "k_gs_select's launch")
    c["select_wide_levels"], c["select_wide"], c["select_narrow"] = int(lvl), int(wide), int(narrow)
    assert "fb += (c + kGsTile - 1u) / kGsTile;" in dev and "next.push_back(c - c / 2u); next.push_back(c / 2u);" in dev
    assert "dim3(kGsPartThreads)" in dev
    # the workgroup's tables
    lds = _body(tree, r"struct SsnTreeLds \{", r"\n\};")
    c["leaf_div"] = int(_one(r"static constexpr int S = B / (\d+);", lds, "SsnTreeLds::S"))
    c["thread_div"] = int(_one(r"static constexpr int T = B / (\d+);", lds, "SsnTreeLds::T"))
    assert "__launch_bounds__(B / %d) void k_ssn_tree(" % c["thread_div"] in tree
    # knn
    c["knn_max"] = int(_one(r"constexpr int kSsnMaxKnn = (\d+);", ssn, "kSsnMaxKnn"))
    lo = _one(r"if \(knn < (\d+) \|\| knn > kSsnMaxKnn\) \{ h->err = \"filter_reference: knn must be in \[3, 32\]\"", icp, "filter_reference's knn range")
    c["knn_min"] = int(lo)
    return c


# the constants as they are today: the tables below are written with them, test_sizes_reach_what_the_tables_claim compares
ROOTS = (2048, 4096, 8192)
ROOT_FROM = {4096: 200 * 4096, 8192: 200 * 8192}
LEAF_FLOOR = 8                      # 8 << root_levels < root_max: a root of B points holds log2(B / 8) levels
GS_TILE, GS_CAND_CAP, GS_PART_THREADS = 2048, 2048, 512
SELECT_WIDE_LEVELS, SELECT_WIDE, SELECT_NARROW = 3, 1024, 256
KNN_MIN, KNN_MAX = 3, 32
# knn 3 is depth-bound at every size, by two levels at a full root -- but its boxes hold two or three points, and a box of two has
# no normal: at the sizes near a power of two (most of the table) the filter keeps a handful of points and a comparison of
# its output says next to nothing about the tree.  knn 4 is depth-bound too (by one level at a full root) and keeps its boxes.
KNNS = (3, 4, 10, 32)
DEVICE_POINTER_KNN = 10             # the knn of the run on device pointers, at B + 1
KINDS = ("smooth", "quantised", "sheet")


def root_auto(n):
    """The root size the library takes by itself"""
    return 8192 if n >= ROOT_FROM[8192] else 4096 if n >= ROOT_FROM[4096] else 2048


def halve(sizes):
    out = []
    for c in sizes:
        out += [c - c // 2, c // 2]
    return out


def shape(n, knn, root, c=None):
    """The host plan of ssn_device restated -> dict(levels, glevels, rem, root_levels, roots: the sizes of the roots in order,
    root_min, root_max, segs: per global level the sizes of its segments, blocks: per global level the kGsTile blocks of each
    segment, empty: leaf slots that stay empty (segments that finished early), depth_bound: did the depth clause ask for a
    global level that the size clause did not, narrow_select: global levels run by the 256-thread k_gs_select)"""
    c = c or dict(leaf_floor=LEAF_FLOOR, gs_tile=GS_TILE, select_wide_levels=SELECT_WIDE_LEVELS)
    levels, k = 0, n
    while k > knn:
        k -= k // 2
        levels += 1
    root_levels = 0
    while (c["leaf_floor"] << root_levels) < root:
        root_levels += 1
    glevels, k = 0, n
    while glevels < levels and not (k <= root and levels - glevels <= root_levels):
        k -= k // 2
        glevels += 1
    by_size, k = 0, n               # the global levels the size clause alone would ask for
    while by_size < levels and k > root:
        k -= k // 2
        by_size += 1
    segs, sizes = [], [n]
    for _ in range(glevels):
        assert min(sizes) > knn, (n, knn, root)       # (a global level halves every one of its segments)
        segs.append(tuple(sizes))
        sizes = halve(sizes)
    roots = tuple(sizes)
    rem = levels - glevels
    for _ in range(rem):            # inside the workgroups: a finished segment carries over, its sibling slot stays empty
        nxt = []
        for s in sizes:
            nxt += [s - s // 2, s // 2] if s > knn else [s, 0]
        sizes = nxt
    empty = sum(1 for s in sizes if s == 0)
    assert len(sizes) == 1 << levels and sum(sizes) == n and max(sizes) <= knn
    tile = c["gs_tile"]
    return dict(levels=levels, glevels=glevels, rem=rem, root_levels=root_levels, roots=roots, root_min=min(roots), root_max=max(roots),
                segs=segs, blocks=[tuple(-(-s // tile) for s in lv) for lv in segs], empty=empty, depth_bound=glevels > by_size,
                narrow_select=max(0, glevels - c["select_wide_levels"]))


def brief(s):
    """What a worker's line and the log say about a shape"""
    return dict(levels=s["levels"], glevels=s["glevels"], rem=s["rem"], root_min=s["root_min"], root_max=s["root_max"], empty=s["empty"],
                depth_bound=s["depth_bound"], blocks=[sorted(set(b)) for b in s["blocks"]])


def sizes(root, knn):
    """The cloud sizes of a root size B and a knn, with what each is there for"""
    b = root
    return {
        knn: "a single box: no level",
        knn + 1: "one level",
        65: "a second wave of the workgroup",
        513: "a second 512-position slab of a wave",
        b - 1: "a root one short of full",
        b: "a full root",
        b + 1: "the first global level",
        2 * b: "two full roots",
        2 * b + 1: "two global levels",
        4 * b + 3: "uneven roots",
        5 * b + 1777: "leaf slots that stay empty",
        16 * b + 5: "global levels run by the 256-thread k_gs_select",
    }


def table():
    """-> [(B, knn, n)] in the order the workers walk it"""
    return [(b, knn, n) for b in ROOTS for knn in KNNS for n in sizes(b, knn)]


# (B, n, knn) -> (levels, glevels, rem, smallest root, largest root, empty leaf slots, depth clause bound): the rows the issue
# states, as the plan restated gives them
CLAIMED = {
    (8192, 8192, 10): (10, 0, 10, 8192, 8192, 0, False),
    (8192, 8193, 10): (10, 1, 9, 4096, 4097, 0, False),
    (8192, 131077, 10): (14, 5, 9, 4096, 4097, 0, False),
    (8192, 8192, 3): (12, 2, 10, 2048, 2048, 0, True),
    (2048, 2048, 3): (10, 2, 8, 512, 512, 0, True),
    (2048, 2049, 32): (7, 1, 6, 1024, 1025, 63, False),
    (4096, 4097, 32): (8, 1, 7, 2048, 2049, 127, False),
    (8192, 8193, 32): (9, 1, 8, 4096, 4097, 255, False),
    (2048, 4097, 10): (9, 2, 7, 1024, 1025, 0, False),
    (8192, 5 * 8192 + 1777, 10): (13, 3, 10, 5342, 5343, 2319, False),
}


# ------------------------------------------------------------------------------------------------ clouds
def cloud(kind, n):
    """-> (n, 4) float32, read-only use; seeded by (kind, n)"""
    rng = np.random.default_rng([KINDS.index(kind), n])
    p = np.ones((n, 4), F)
    if kind == "smooth":
        # per axis a point per cell of extent / n, at most half a cell from the cell's start: distinct after rounding to float32
        for d, ext in enumerate((60.0, 35.0, 8.0)):
            p[:, d] = ((rng.permutation(n) + 0.5 * rng.random(n)) * (ext / n) - ext / 2).astype(F)
        return p
    p[:, :3] = (np.round(rng.normal(size=(n, 3)) * np.array([40.0, 25.0, 6.0])) / 4).astype(F)
    if kind == "sheet":
        p[:, 2] = F(1.5)
    return p


def order_key(f):
    """float_order_key of csrc: unsigned keys in the order of the floats, -0 as +0"""
    u = np.ascontiguousarray(f, F).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where((u & 0x80000000) != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def cut_axis(lo, hi):
    """The widest axis in float32, the first of equal ones"""
    ext = (hi - lo).astype(F)
    cut = 0
    if ext[1] > ext[0]:
        cut = 1
    if ext[2] > ext[cut]:
        cut = 2
    return cut


def median_ties(p, knn, nlevels):
    """The chain of stable sorts down `nlevels` levels -> per level the number of segments whose median lies inside a run of
    equal cut coordinates (the key left of the cut equals the key right of it): where the stable order decides which
    points go left."""
    keys = [order_key(p[:, d]) for d in range(3)]
    lo, hi = p[:, :3].min(0), p[:, :3].max(0)
    segs = [(np.arange(len(p)), lo, hi)]
    out = []
    for _ in range(nlevels):
        ties, nxt = 0, []
        for order, lo, hi in segs:
            c = len(order)
            assert c > knn
            a = cut_axis(lo, hi)
            o2 = order[np.argsort(keys[a][order], kind="stable")]
            left = c - c // 2
            ties += int(keys[a][o2[left - 1]] == keys[a][o2[left]])
            cutval = p[o2[left], a]
            hi2, lo2 = hi.copy(), lo.copy()
            hi2[a] = cutval
            lo2[a] = cutval
            nxt += [(o2[:left], lo, hi2), (o2[left:], lo2, hi)]
        out.append(ties)
        segs = nxt
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
