"""The reference filter's box tree (SamplingSurfaceNormalDataPointsFilter on the device) at every root size and tree shape:
the sort-free upper levels (csrc/lsgpu_ssn_select.hip.h), the segmented-sort levels they fall back to, and k_ssn_tree<B>
(csrc/lsgpu_ssn_tree.hip.h) with B = 2048, 4096 and 8192 points per workgroup, through filter_reference against the oracle,
bit for bit.  tests/ssn_cases.py has the sizes, what each reaches (the host plan of ssn_device restated) and the clouds;
tests/ssn_worker.py is the process that runs under LSGPU_SSN_ROOT / LSGPU_SSN_SORT_LEVELS.

CPU part (no marker): the size tables against the constants parsed from the sources and against the rows they were written
with; the host twin against the oracle on the whole table; the numpy models of tests/ssn_tree_model.py (presorted_lists,
select_then_tree) against the chain of stable sorts on the tie clouds at 513 to 4097 points (tests/test_oracle.py draws
fewer than 400); the clouds are what they claim: `quantised` and `sheet` put a run of equal coordinates across the median
of the root and of a segment of every global level, `smooth` has no two equal coordinates.

Device part: five child processes (the LSGPU_* switches are read once), LSGPU_SSN_ROOT = 2048 / 4096 / 8192,
LSGPU_SSN_SORT_LEVELS at the default root, and both at 8192.  Each walks its B's table -- 12 sizes x knn 3, 4, 10, 32 x 3
clouds, 144 cases, each at ratio 1 and at ratio 0.4 with the draw stream's position behind it, 289 calls of the filter --
and ends with the handle's counters: ssn_calls equal to the calls made and ssn_sort_fallbacks 0, since a filter that gave
up and ran again with the segmented sorts is still bit-exact and would otherwise pass.  A worker that dies, reports a HIP
error or overruns its limit fails its test and nothing further is started on the device: the remaining device tests skip,
naming it.

The output is the kept points in ascending original index with their box's normal.  At ratio 1 it shows which box a point
is in; the order inside a box shows only at ratio 0.4, where a point's draw is the one of its place in the traversal.  The
ratio 0.4 runs are therefore made for every knn on every cloud (a worker takes seconds), not for knn 10 alone.

Where the table differs from what it was asked to hold.  No cloud gives k_ssn_tree<8192>'s plan a global segment of
exactly kGsTile or kGsTile + 1 points: 2048 points with knn 3 need ten levels, which a root of 8192 holds, so a segment
that small is a root, not a global segment.  For B = 8192 the CPU test asserts that this is so, and that the table holds
what the pair of sizes is there for at the sizes that do occur: a global segment of whole blocks (16 384: eight) and one
with a single point in its last block (8193: four blocks and a point).  knn 4 is added to 3, 10 and 32: the depth-bound plan
is knn 3's everywhere, but boxes of two points have no normal, and at the sizes near a power of two -- most of the table --
knn 3 keeps a handful of points (15 of 32 773): the comparison there sees almost nothing of the tree.  knn 4 is depth-bound
as well and keeps its boxes.

Seen on an MI355X: all five workers pass, 144 cases and 289 filter calls each, ssn_calls 289 and ssn_sort_fallbacks 0 in
every one; nothing on stderr names LSGPU_SSN_ROOT.  No defect was found in csrc/; the one change there is the comment of
lsgpu_tuning.h that gave LSGPU_SSN_ROOT's default as 8192 (it is by size).

With the step of k_ssn_tree's level loop that moves tie runs into the segment's current order taken out of a scratch build
(fix[k] false: every list stays a permutation, only orders go wrong), the B = 2048 worker, run once: `smooth` passes all 48
cases; `quantised` fails 33 of 48 and `sheet` 31 of 48.  Of the cases with more than one level that pass, all but one are
knn 3's (0 to 12 points kept: nothing to compare) -- knn 3 fails 4 of 12 on `quantised` and 2 of 12 on `sheet`, knn 4 and
knn 10 fail 10 of 12 on both, every size from 65 points on -- and the other is 65 points with knn 32, two levels.  17 of
`sheet`'s 31 failures show at ratio 0.4 only (boxes right, order inside them wrong), 10 of them at knn 3, 4 and 32.

Wall time on an MI355X: 19 s for the five device tests -- 2.7 s (LSGPU_SSN_ROOT 2048; 0.9 s of it inside the worker), 3.6 s
(4096; 1.6 s), 5.0 s (8192; 3.0 s), 3.0 s (LSGPU_SSN_SORT_LEVELS; 0.9 s), 4.7 s (both; 2.9 s), the rest interpreter start and
library load; a case takes 0.5 ms at 65 points and 0.1 s at 131 077, most of it the oracle.  About 25 s for the CPU part on one
core: 3.5 s the oracle on the whole table (shared), 8 s the host twin, 3.7 s the tie runs of the clouds, 4 s the models.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ssn_cases as sc
from test_primitive_sizes import WORKER_TIMEOUT     # s: interpreter start, library load, the checked sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MODEL_SIZES = (513, 2047, 2048, 2049, 4097)
MODEL_KNNS = (3, 10)
# name -> (LSGPU_SSN_ROOT or None, LSGPU_SSN_SORT_LEVELS)
WORKERS = {"root2048": (2048, False), "root4096": (4096, False), "root8192": (8192, False), "sort_levels": (None, True),
           "root8192_sort_levels": (8192, True)}


def all_sizes():
    """Every (n, knn) of the three tables, once"""
    return sorted({(n, knn) for _b, knn, n in sc.table()})


# ------------------------------------------------------------------------------------------------ the tables, on the CPU
def test_sizes_reach_what_the_tables_claim():
    c = sc.constants()
    assert c["roots"] == sc.ROOTS and c["root_from"] == sc.ROOT_FROM == {4096: 819200, 8192: 1638400}
    assert c["leaf_floor"] == sc.LEAF_FLOOR == c["leaf_div"] == c["thread_div"]     # B / 8 leaf slots, B / 8 threads
    assert c["tree_threads"] == {b: b // c["thread_div"] for b in sc.ROOTS}
    assert (c["gs_tile"], c["gs_cand_cap"], c["gs_part_threads"]) == (sc.GS_TILE, sc.GS_CAND_CAP, sc.GS_PART_THREADS)
    assert (c["select_wide_levels"], c["select_wide"], c["select_narrow"]) == (sc.SELECT_WIDE_LEVELS, sc.SELECT_WIDE, sc.SELECT_NARROW)
    assert (c["knn_min"], c["knn_max"]) == (sc.KNN_MIN, sc.KNN_MAX) and set(sc.KNNS) >= {sc.KNN_MIN, 10, sc.KNN_MAX}
    assert all(sc.KNN_MIN <= k <= sc.KNN_MAX for k in sc.KNNS)
    # the rows the tables were written with
    for (b, n, knn), want in sc.CLAIMED.items():
        s = sc.shape(n, knn, b, c)
        got = (s["levels"], s["glevels"], s["rem"], s["root_min"], s["root_max"], s["empty"], s["depth_bound"])
        print("B", b, "n", n, "knn", knn, got, "claimed", want)
        assert got == want, (b, n, knn)
        assert knn in sc.KNNS and n in sc.sizes(b, knn)
    s = sc.shape(4097, 10, 2048, c)
    assert s["segs"][1] == (2049, 2048) and s["blocks"][1] == (2, 1)
    tile = c["gs_tile"]
    for b in sc.ROOTS:
        log2 = b.bit_length() - 1
        assert 1 << log2 == b
        for knn in sc.KNNS:
            assert list(sc.sizes(b, knn)) == [knn, knn + 1, 65, 513, b - 1, b, b + 1, 2 * b, 2 * b + 1, 4 * b + 3, 5 * b + 1777, 16 * b + 5]
            assert len(set(sc.sizes(b, knn))) == 12
        rows = {(n, knn): sc.shape(n, knn, b, c) for bb, knn, n in sc.table() if bb == b}
        for (n, knn), s in rows.items():
            print("B", b, "n", n, "knn", knn, sc.brief(s), "--", sc.sizes(b, knn)[n])
            assert sc.root_auto(n) == sc.ROOTS[0]                   # only LSGPU_SSN_ROOT reaches the two larger instantiations here
            assert s["root_max"] <= b and s["rem"] <= log2 - 3 == s["root_levels"] and s["levels"] == s["glevels"] + s["rem"]
            assert len(s["roots"]) == 1 << s["glevels"] and sum(s["roots"]) == n
            assert (s["levels"] == 0) == (n <= knn) and (n != knn + 1 or s["levels"] == 1)
        every = rows.values()
        assert any(s["root_max"] == b for s in every) and any(s["root_max"] == b - 1 for s in every)
        assert any(s["root_min"] == s["root_max"] == b and s["glevels"] == 1 for s in every)                # two full roots
        assert any(s["root_min"] < s["root_max"] for s in every)
        assert {0, 1} <= {s["glevels"] for s in every} and any(s["glevels"] >= 4 for s in every)
        assert any(s["narrow_select"] >= 2 for s in every)                                            # the 256-thread k_gs_select
        assert any(s["narrow_select"] and min(s["segs"][-1]) <= 2 * tile for s in every)              # ... on small segments
        assert any(s["depth_bound"] for s in every) and any(s["empty"] for s in every)
        assert any(s["depth_bound"] and s["root_max"] * 4 <= b for s in every)                        # knn 3: roots of a quarter
        assert any(s["rem"] == s["root_levels"] and s["root_max"] == b for s in every)
        segs = {v for s in every for lv in s["segs"] for v in lv}
        assert any(v % tile == 0 for v in segs) and any(v % tile == 1 and v > tile for v in segs)
        if b < 8192:
            assert tile in segs and tile + 1 in segs
        else:   # a segment that small is a root whatever knn: see the docstring
            assert sc.shape(tile, sc.KNN_MIN, b, c)["glevels"] == 0 and sc.shape(tile + 1, sc.KNN_MIN, b, c)["glevels"] == 0
            assert 8 * tile in segs and 4 * tile + 1 in segs
    assert rows[(5 * 8192 + 1777, 10)]["empty"] == 2319
    assert sc.shape(2048, 3, 2048, c)["root_max"] == 512 and c["tree_threads"][8192] == 1024          # 512-point roots exist; 1024 threads
    assert sc.shape(8192, 3, 8192, c)["root_max"] == 2048


@pytest.fixture(scope="module")
def references(oracle):
    """(n, knn, kind) -> the oracle's (points, normals) at ratio 1, for the whole table; read-only"""
    out = {}
    t0 = time.perf_counter()
    for n, knn in all_sizes():
        for kind in sc.KINDS:
            of, on = oracle.sampling_surface_normal(sc.cloud(kind, n), knn, 1.0, 2)
            of.setflags(write=False); on.setflags(write=False)
            out[(n, knn, kind)] = (of, on)
    print("the oracle on the whole table: %.2f s" % (time.perf_counter() - t0))
    return out


@pytest.mark.parametrize("knn", sc.KNNS)
def test_host_twin_equals_the_oracle_on_the_whole_table(knn, oracle, references):
    from laser_slam_amd import icp
    for (n, k, kind), (of, on) in references.items():
        if k != knn:
            continue
        p = sc.cloud(kind, n)
        hf, hn = icp.sampling_surface_normal(p, knn, 1.0, 2)
        assert sc.same(hf, of) and sc.same(hn, on), (n, knn, kind)
        if kind == "quantised":
            of4, on4 = oracle.sampling_surface_normal(p, knn, 0.4, 7)
            hf4, hn4 = icp.sampling_surface_normal(p, knn, 0.4, 7)
            assert sc.same(hf4, of4) and sc.same(hn4, on4) and (len(of) < 200 or 0.25 * len(of) < len(of4) < 0.55 * len(of)), (n, kind)


def test_the_table_compares_more_than_a_handful_of_points(references):
    """What a bit-exact comparison of the output can see: the points of boxes that have a normal.  knn 3 leaves boxes of two
    points at most sizes (ssn_cases.KNNS); every depth-bound size from B - 1 on is also run with knn 4, which keeps them."""
    for b in sc.ROOTS:
        for knn in sc.KNNS:
            for n in sc.sizes(b, knn):
                kept = {kind: len(references[(n, knn, kind)][0]) for kind in sc.KINDS}
                s = sc.shape(n, knn, b)
                if knn == 3 and n >= b - 1:
                    print("B", b, "n", n, "knn 3 keeps", kept)
                # in general position a box of three points or more has a normal, one of two has none
                assert kept["smooth"] == sum(v for v in _leaf_sizes(n, knn) if v >= 3), (b, n, knn, kept)
                # knn 4: the worst a cloud can do is segments of five points throughout, 3 + 2 each: three fifths are kept
                # (a sheet's boxes are flat and those with all points in a line are dropped: 131 077 points on some 36 000 grid
                #  nodes leave a box of four with a normal one time in ten)
                if knn >= 4 and n >= 65:
                    assert kept["smooth"] >= 0.6 * n and kept["quantised"] > 0.5 * n and kept["sheet"] > 0.05 * n, (b, n, knn, kept)
                if knn >= 10 and n >= 65:
                    assert kept["smooth"] == n, (b, n, knn, kept)
                if knn == 4 and n >= b - 1:
                    assert s["depth_bound"], (b, n)
    assert len(references[(32773, 3, "smooth")][0]) < 100


@pytest.mark.parametrize("kind", ("quantised", "sheet"))
@pytest.mark.parametrize("n", MODEL_SIZES)
def test_tree_models_equal_the_chain_of_stable_sorts_on_tie_clouds(n, kind):
    """presorted_lists (k_ssn_tree's scheme) and select_then_tree (the sort-free levels down to the roots the device would
    build with B = 2048, k_ssn_tree's scheme below) give the leaves of the chain of stable sorts, in the same order inside
    every leaf."""
    import ssn_tree_model as M
    pts = sc.cloud(kind, n)[:, :3].copy()
    lo, hi = pts.min(0), pts.max(0)
    for knn in MODEL_KNNS:
        s = sc.shape(n, knn, 2048)
        a = M.chain_of_stable_sorts(pts, knn, lo, hi)
        b = M.presorted_lists(pts, knn, lo, hi)
        c = M.select_then_tree(pts, knn, lo, hi, s["root_max"])
        assert [len(x) for x in a] == _leaf_sizes(n, knn)
        for other in (b, c):
            assert len(other) == len(a), (n, knn, kind)
            assert all(np.array_equal(x, y) for x, y in zip(a, other)), (n, knn, kind)


def _leaf_sizes(n, knn):
    sizes = [n]
    while max(sizes) > knn:
        sizes = [v for s in sizes for v in ((s - s // 2, s // 2) if s > knn else (s,))]
    return sizes


def test_the_clouds_are_what_they_claim():
    for n, knn in all_sizes():
        for kind in sc.KINDS:
            p = sc.cloud(kind, n)
            assert p.dtype == F and p.shape == (n, 4) and np.all(p[:, 3] == 1) and np.isfinite(p).all()
            assert np.array_equal(p, sc.cloud(kind, n))                                     # seeded by (kind, n)
        smooth, quantised, sheet = (sc.cloud(kind, n) for kind in sc.KINDS)
        for d, ext in enumerate((60.0, 35.0, 8.0)):
            assert len(np.unique(smooth[:, d])) == n and np.abs(smooth[:, d]).max() <= ext / 2
        assert np.array_equal(quantised[:, :3] * 4, np.round(quantised[:, :3] * 4))
        assert np.all(sheet[:, 2] == F(1.5)) and np.array_equal(sheet[:, :2] * 4, np.round(sheet[:, :2] * 4))
        if n >= 4096:
            assert (smooth[:, 0] < 0).any() and (smooth[:, 0].max() - smooth[:, 0].min()) > 59
    # runs of equal coordinates across the medians: with numpy on the keys, down the global levels of every B
    for b in sc.ROOTS:
        for knn in sc.KNNS:
            for n in sc.sizes(b, knn):
                if n < 2049:
                    continue
                nlevels = max(sc.shape(n, knn, b)["glevels"], 1)
                for kind in ("quantised", "sheet"):
                    ties = sc.median_ties(sc.cloud(kind, n), knn, nlevels)
                    assert ties[0] == 1 and min(ties) >= 1, (b, n, knn, kind, ties)
                assert sc.median_ties(sc.cloud("smooth", n), knn, nlevels) == [0] * nlevels, (b, n, knn)


# ------------------------------------------------------------------------------------------------ the device runs
_STOPPED = None     # why nothing further is started on the device


def _device_or_skip():
    if _STOPPED:
        pytest.skip("nothing more on the device after " + _STOPPED)


@pytest.mark.gpu
@pytest.mark.timeout(180)
@pytest.mark.parametrize("name", list(WORKERS))
def test_reference_filter_at_every_root_size_and_tree_shape(name):
    """tests/ssn_worker.py with the environment of WORKERS[name] (and no other LSGPU_SSN_* switch)."""
    global _STOPPED
    _device_or_skip()
    root, sort_levels = WORKERS[name]
    b = root or sc.ROOTS[0]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSGPU_SSN_")}
    if root:
        env["LSGPU_SSN_ROOT"] = str(root)
    if sort_levels:
        env["LSGPU_SSN_SORT_LEVELS"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ssn_worker.py")]
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STOPPED = f"the worker {name} overran its {WORKER_TIMEOUT} s"
        pytest.fail(_STOPPED)
    res = [json.loads(ln[len("SSN_RESULT "):]) for ln in p.stdout.splitlines() if ln.startswith("SSN_RESULT ")]
    done = [json.loads(ln[len("SSN_DONE "):]) for ln in p.stdout.splitlines() if ln.startswith("SSN_DONE ")]
    hip = [r for r in res if r.get("code") == 3]
    if hip:
        _STOPPED = f"a HIP error in the worker {name}, {hip[0]['n']} points, knn {hip[0]['knn']}, {hip[0]['kind']}"
        pytest.fail(f"{_STOPPED}: {hip[0]}")
    if p.returncode != 0 or len(done) != 1:
        _STOPPED = f"the worker {name} ended with status {p.returncode}"
        pytest.fail(f"{_STOPPED}\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
    done = done[0]
    print("worker", name, "%.2f s in the worker, %.2f s in all," % (done["seconds"], time.perf_counter() - t0), done["calls"], "calls,",
          "ssn_calls", done.get("ssn_calls"), "ssn_sort_fallbacks", done.get("ssn_sort_fallbacks"))
    for r in res:
        why = sc.sizes(b, r["knn"])[r["n"]]
        claimed = sc.CLAIMED.get((b, r["n"], r["knn"]))
        print("B", b, "n", r["n"], "knn", r["knn"], r["kind"], r["shape"], "kept", r.get("kept"), "%.3f s" % r.get("seconds", -1.0), "--", why,
              *(("claimed", claimed) if claimed else ()))
    assert "LSGPU_SSN_ROOT" not in p.stderr, p.stderr[-1500:]     # (the library says so when it does not take the value)
    assert done["b"] == b and done["sort_levels"] == sort_levels
    want = [(n, knn, kind) for bb, knn, n in sc.table() if bb == b for kind in sc.KINDS]
    assert [(r["n"], r["knn"], r["kind"]) for r in res] == want and done["cases"] == len(want)
    bad = []
    for r in res:
        assert "error" not in r, r
        assert r["shape"] == sc.brief(sc.shape(r["n"], r["knn"], b)), r
        if r["failures"]:
            bad.append((b, r["n"], r["knn"], r["kind"], r["shape"]["levels"], r["shape"]["glevels"], r["shape"]["rem"], r["failures"]))
    assert not bad, bad
    # a filter that gave up ran again with the segmented sorts and is bit-exact all the same: only the counter shows it
    assert done["ssn_sort_fallbacks"] == 0 and done["ssn_calls"] == done["calls"], done
