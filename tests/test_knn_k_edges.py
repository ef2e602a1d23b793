"""The k-nearest search (csrc/lsgpu_knn_k.hip.h) at every k, on exact ties, far queries, lists a maxDist leaves partly empty,
a cell of more than 64 chunks, query counts at the edges of a wave and a block, and references of k and k + 1 points.
tests/knn_k_cases.py has the builders, the constants parsed from the sources and the tie-set rule.

The reference everywhere is the brute force of tests/cpp/knn_brute.c (the device's float arithmetic, ascending (d2, input
index)), masked by maxDist as tests/test_outlier_chain.py masks it.  Distances are compared bit for bit; ids through
_check_knn_k of test_outlier_chain.py (equal up to exact ties, the named point at exactly the reported distance, invalid
entries last) and through kc.check_tie_sets: the two orders differ only within one distance value, so below a row's last
distance the SETS of ids at each value are equal.

CPU part (no marker): the parsed constants against the ones the cases were written with; and, on the brute force alone, that
every case contains what it is for -- the lattice's tie multiplicities and, for every k, at least a quarter of its queries
tied across the k-th / (k+1)-th place; at least 1 000 far queries that must go to the fallback and 1 000 the tile can serve;
m valid entries beside the cluster of m points, the lonely and the edge query, 2 to 98 % invalid entries; the dense cube
strictly inside one level-0 cell with more points than 64 chunks hold; k nq on both sides of 256 and of a multiple of it.

Device part -- which instantiations of k_knnk_seed / k_knnk_tile / k_knnk_fallback<K, MAXD> a test launches:
  test_every_instantiation         <K, false>, <K, true> (maxDist 0.5 and 3.25) for K = 1..8: all sixteen.  About 43 % of the
                                   batch goes to the fallback necessarily without a maxDist and under 3.25 m (none under
                                   0.5 m: there every bound is below the cap); under 3.25 m the fallback stores partly
                                   empty lists for K > 1 (the cluster queries, the scan's fringe).
  test_lattice_ties                <K, false> K = 1..8, <K, true> K = 2, 5, 8: tile and fallback on exact ties.
  test_lattice_batch_independence  <K, false / true> K = 2, 5, 8: nq = 1 launches, the reversed batch.
  test_max_dist_beyond_every_answer_changes_nothing   <K, true> K = 1..8 with a bound (100 m) that cuts nothing nearby.
  test_coincident_points_keep_input_order             <K, false> K = 1..8 on a reference with every point twice.
  test_query_counts                <3 / 7, false / true>, nq 1 .. 257.
  test_references_of_k_and_k_plus_one_points           <K, false / true> K = 1..8: the seed's climb to the top level.
  test_dense_cell                  <1 / 4 / 8, false / true>: the second round of the 64-chunk loops, tile and fallback.
The loops at the K no test warm-started are in test_knn_matcher.py (k = 2, 5, 6, 7) and test_outlier_chain.py (the chain
"wide-matcher+trim": maxDist 3.25 m with k = 4 point-to-plane and k = 2 point-to-point).

Coincident points: k_ref_keys (csrc/lsgpu_grid.hip.h) gives a point the Morton key of its quantised coordinates -- all 48 key
bits, nothing of its index -- and its input index as the value; sort_pairs (csrc/lsgpu_sort.hip.h) is a stable LSD radix sort
over all 48 bits.  Coincident points have equal keys, so they keep their input order in the sorted reference, and the
device's tie rule (smaller sorted index) is the brute force's (smaller input index) among them: guaranteed, and tested.

Share of fallback queries: the handle does not report its straggler count, so what is recorded is the share that goes there
NECESSARILY (kc.necessarily_fallback, from the brute force), a lower bound.

Seen on an MI355X: all 74 device tests and the six added loop cases pass (the loops with equal traces and a pose difference
of 0 m / 0 rad); no defect was found in csrc/.  Wall time of the file, CPU part included: 3.4 s for its 83 tests, 1.4 s of it
the first handle; no test takes more than 0.25 s.
  test_every_instantiation, 8 076 queries: 38.6 % (k = 1) to 42.8 % (k = 8) go to the fallback necessarily without a maxDist
      and under 3.25 m, none under 0.5 m; invalid entries 44.8 % (k = 1) to 53.6 % (k = 8) under 0.5 m and 27.7 to 28.3 % under
      3.25 m, where 88 lists of eight are partly empty.  The scan has next to no exact ties: at most 4 ids differ from the brute
      force's; the tie-set rule holds 56 531 of the 64 608 ids at k = 8 to the brute force's outright.
  lattice, 472 queries: 72 (the outside ones) necessarily in the fallback; 7.6 % invalid entries under 3.25 m (the 36 queries
      20 m outside); 293 of 944 ids (k = 2) to 2 122 of 3 776 (k = 8) differ from the brute force's, every one of them a legal
      tie, while the set rule holds 136 to 1 624 ids to the brute force's.
  dense cell, 800 queries, 1 920 chunks: 12.5 % (the 100 queries 5 m off) necessarily in the fallback, all invalid under 3.25 m.
The device's column order among coincident points is not the brute force's column by column (the brute force lists the other
first copies of a tie between a point's two copies): check_copies says what is equal, and
test_the_checks_pass_on_a_model_of_the_device_order runs every check on the CPU against the brute force over the
Morton-sorted reference, which is the device's rule.

That the tests can fail.  Three scratch copies of lsgpu_knn_k.hip.h, each with one rule broken, were compiled for gfx950 and
never run on a device; the broken rules were replayed on the CPU by a port of kbest_before / kbest_insert and of the
fallback's merge over the lattice (72 queries, twelve of every kind, K = 2, 5, 8, points arriving in ascending and in
descending sorted index, the lists starting at the exact k-th distance and at four times it) and the partial-list data, the
results put through the checks of this file:
  kbest_before without its tie clause (d < e alone).  A list starting at a bound that IS the k-th distance -- what a good
      seed gives -- rejects the point at that distance and keeps a sentinel: _check_knn_k fails on d2 in every test of
      the file.  From a wider bound the distances and sets still pass against the brute force, but equal distances stay in
      arrival order: the ids differ between the two arrival orders in all 72 rows -- test_lattice_batch_independence
      (alone, in the batch, reversed) and the repeat in test_lattice_ties are what that leaves.
  one bubble step of kbest_insert left out (the loop ends at s > 1).  The head of a list is never replaced: d2 differs from the
      brute force's in every replayed row, K = 2, 5 and 8 alike -- every comparison of the file with K >= 2.
  the fallback merge reading a sentinel's index as 0 instead of kKnnNoIndex.  At d2 == maxDist^2 the sentinel ranks before the
      real point: the edge query comes back as point 0 at 10.5625 and the lonely query's empty entries as valid ones --
      test_every_instantiation under maxDist 3.25 at every K (the cluster, lonely and edge assertions, and _check_knn_k on
      the scan's fringe), test_lattice_ties, test_dense_cell and test_references_of_k_and_k_plus_one_points under 3.25.
"""
import ctypes as C

import numpy as np
import pytest

import host_loop
import knn_k_cases as kc
from laser_slam_amd import _lib
from test_grid_geometry import predict_geometry
from test_outlier_chain import _check_knn_k, mask_matches

F = np.float32


@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    return host_loop.build_brute(tmp_path_factory.mktemp("knn_brute"))


@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


@pytest.fixture(scope="module")
def handles(icp_mod):
    """One handle per (reference, maxDist) for the whole file: get(name, reference, max_dist, cell_size) -> handle"""
    made = {}

    def get(name, ref, max_dist=None, cell_size=0.0):
        if (name, max_dist) not in made:
            cfg = _lib.IcpConfig()
            _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
            cfg.cell_size = cell_size
            h = icp_mod.IcpHandle(cfg, matcher_max_dist=max_dist)
            made[(name, max_dist)] = h
            h.set_reference(ref, None)
        return made[(name, max_dist)]
    yield get
    for h in made.values():
        h.close()


_cases = {}


def far_case(oracle, pair4k, mean):
    """The partial-list reference (pair4k's reference scan and the clusters) centred on `mean`, and the batch: the far
    queries, then the cluster, lonely and edge queries -> dict(ref, ref_c, at, q, n_far, rows: name -> row of q)"""
    key = ("far", np.asarray(mean, F).tobytes())
    if key not in _cases:
        ref, at = kc.partial_reference(pair4k)
        ref_c = kc.centred(ref, mean)
        far = kc.far_batch(oracle, pair4k, mean)
        pq, rows = kc.partial_queries(ref_c, at)
        _cases[key] = dict(ref=ref, ref_c=ref_c, at=at, q=np.concatenate([far, pq]), n_far=len(far),
                           rows={name: len(far) + r for name, r in rows.items()})
    return _cases[key]


def lattice_case(n=kc.LATTICE_N, copies=1):
    key = ("lattice", n, copies)
    if key not in _cases:
        q, kind = kc.lattice_queries(n=n)
        _cases[key] = dict(ref=kc.lattice(copies, n), q=q, kind=kind)
    return _cases[key]


def dense_case():
    if "dense" not in _cases:
        ref, cube, lo = kc.dense_reference()
        q, group = kc.dense_queries(lo)
        _cases["dense"] = dict(ref=ref, cube=cube, lo=lo, q=q, group=group, geom=predict_geometry(ref, kc.DENSE_CELL_SIZE))
    return _cases["dense"]


def check(ids, d2, bids, bd2, ref_c, q):
    _check_knn_k(ids, d2, bids, bd2, ref_c, q)
    return kc.check_tie_sets(ids, d2, bids, bd2)


# ------------------------------------------------------------------------------------------------ CPU: the cases hold what they are for
def test_constants_are_what_the_cases_were_built_for():
    c = kc.constants()
    assert (c["r_cap"], c["chunk_max"], c["knn_max"]) == (kc.R_CAP, kc.CHUNK_MAX, kc.KNN_MAX)
    assert (c["tile_wave"], c["seed_block"], c["unpermute_block"], c["cell_round"]) == \
        (kc.TILE_WAVE, kc.SEED_BLOCK, kc.UNPERMUTE_BLOCK, kc.CELL_ROUND)
    assert kc.KS == tuple(range(1, 9)) and _lib.MATCHER_KNN_MAX == kc.KNN_MAX
    assert kc.sq(kc.MAX_DIST_WIDE) == F(10.5625) and kc.sq(kc.MAX_DIST_NEAR) == F(0.25)
    # a bound cut to maxDist 0.5 never reaches the cap, one cut to 3.25 does: sqrt(ub) (1 + 1e-5) + 1e-7 + kFineSlack hf
    hf = 0.125 / 32
    assert kc.MAX_DIST_NEAR * (1 + 1e-5) + 1e-7 + c["fine_slack"] * hf < c["r_cap"] < kc.MAX_DIST_WIDE


def test_check_tie_sets_tells_a_legal_tie_from_a_wrong_point():
    d2 = F([[0.0, 0.25, 0.25, 0.5], [0.1, 0.2, 0.2, np.inf]])
    bids = np.int32([[5, 1, 2, 9], [4, 6, 7, -1]])
    ok = np.int32([[5, 2, 1, 11], [4, 7, 6, -1]])                    # permuted within 0.25; another point at the last value
    assert kc.check_tie_sets(ok, d2, bids, d2) == 3 + 3
    for bad in (np.int32([[5, 1, 3, 9], [4, 6, 7, -1]]),             # a wrong point below the last distance
                np.int32([[5, 1, 2, 9], [4, 6, 8, -1]])):            # a wrong point at the last value of a list with room left
        with pytest.raises(AssertionError):
            kc.check_tie_sets(bad, d2, bids, d2)


def test_lattice_case_has_its_ties(brute):
    c = lattice_case()
    ref, q, kind = c["ref"], c["q"], c["kind"]
    assert len(ref) == 17 ** 3 and (ref[:, :3].astype(np.float64).sum(0) == 0).all()        # the mean is 0: centred == given
    assert (np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] == 0).all()
    assert (predict_geometry(ref)["mean"] == 0).all()
    _ids, d2 = brute(ref, q, 16)
    for what, shells in kc.LATTICE_TIES.items():
        rows = d2[kind == what]
        assert 95 <= len(rows) <= 110
        at = 0
        for dist, mult in shells:
            assert (rows[:, at:at + mult] == F(dist)).all(), (kc.KIND_NAMES[what], dist)
            assert (rows[:, at + mult] > F(dist)).all(), (kc.KIND_NAMES[what], dist, mult)
            at += mult
    for dist in kc.OUTSIDE:                                          # one nearest point, then four a step aside; or four at once
        on, off = d2[(kind == kc.OUT_ON) & (d2[:, 0] == F(dist * dist))], d2[kind == kc.OUT_OFF]
        assert len(on) == 18 and (on[:, 1:5] == F(dist * dist + 0.25)).all() and (on[:, 5] > on[:, 4]).all()
        off = off[off[:, 0] == F(dist * dist + 0.125)]
        assert len(off) == 18 and (off[:, :4] == off[:, :1]).all() and (off[:, 4] > off[:, 3]).all()
    assert (kc.necessarily_fallback(d2[:, 0])).sum() == 72 == (kind >= kc.OUT_ON).sum()
    d9 = brute(ref, q, 9)[1]
    assert np.array_equal(d9, d2[:, :9])
    for k in kc.KS:
        assert kc.tie_share(d9, k) >= 0.25, (k, kc.tie_share(d9, k))
    # the doubled lattice of the coincident-points test: the same, smaller
    c2 = lattice_case(6, 2)
    assert len(c2["ref"]) == 2 * 13 ** 3 and np.array_equal(c2["ref"][:13 ** 3], c2["ref"][13 ** 3:])
    assert (c2["ref"][:, :3].astype(np.float64).sum(0) == 0).all()


def test_the_checks_pass_on_a_model_of_the_device_order(brute):
    """The device's rule, (d2, index in the Morton-sorted reference), is the brute force's rule on the reference in that
    order: kc.sorted_order restates k_ref_keys and the stable sort.  On the lattice and on the lattice with every point twice
    the model's answers pass every check the device's are put through, check_copies at every k included -- the checks ask
    nothing of a correct search that ties make impossible."""
    for n_half, copies in ((kc.LATTICE_N, 1), (6, 2)):
        c = lattice_case(n_half, copies)
        ref, q = c["ref"], c["q"]
        order = kc.sorted_order(ref)
        for k in kc.KS:
            sid, d2 = brute(ref[order], q, k)
            ids = order[sid].astype(np.int32)
            bids, bd2 = brute(ref, q, k)
            check(ids, d2, bids, bd2, ref, q)
            assert (ids != bids).any() or k == 1
            if copies == 2:
                check_copies(ids, bids, len(ref) // 2)


def test_far_case_reaches_the_fallback_and_the_tile(oracle, brute, pair4k):
    c = far_case(oracle, pair4k, kc.mean_of(kc.partial_reference(pair4k)[0]))
    ref_c, q, at, rows = c["ref_c"], c["q"], c["at"], c["rows"]
    assert len(ref_c) <= 8000 and len(q) <= 8200
    bids, bd2 = brute(ref_c, q, 8)
    far = bd2[:c["n_far"]]
    assert (far[:, 1] > F(kc.R_CAP ** 2)).sum() >= 1000              # k = 2 and up: to the fallback necessarily
    assert (far[:, 7] < F(0.25 ** 2)).sum() >= 1000                  # every k: a ball the tile can serve
    for k in kc.KS:
        for md in kc.MAX_DISTS:
            print("k", k, "maxDist", md, "necessarily fallback %.3f" % kc.necessarily_fallback(bd2[:, k - 1], md).mean(),
                  "invalid entries %.3f" % np.isinf(mask_matches(bids[:, :k], bd2[:, :k], md)[1]).mean())
    # every cluster stands alone
    own = np.concatenate([at[m] for m in kc.CLUSTERS])
    for m in kc.CLUSTERS:
        others = np.delete(np.arange(len(ref_c)), at[m])
        d = np.linalg.norm(ref_c[at[m], None, :3].astype(np.float64) - ref_c[None, others, :3], axis=2)
        assert d.min() >= kc.CLUSTER_CLEAR, (m, d.min())
    assert len(own) == 28
    # under maxDist 3.25: m valid entries beside cluster m, none for the lonely query, the edge query at exactly 3.25 m
    mids, md2 = mask_matches(bids, bd2, kc.MAX_DIST_WIDE)
    for m in kc.CLUSTERS:
        r = rows[m]
        assert np.isfinite(md2[r]).sum() == m and np.array_equal(mids[r, :m], at[m]) and (np.diff(md2[r, :m]) > 0).all()
    assert np.isinf(md2[rows["lonely"]]).all()
    assert md2[rows["edge"], 0] == F(10.5625) and mids[rows["edge"], 0] == at[1][0] and np.isinf(md2[rows["edge"], 1])
    for md in (kc.MAX_DIST_NEAR, kc.MAX_DIST_WIDE):
        for k in (1, 8):
            inv = np.isinf(mask_matches(bids[:, :k], bd2[:, :k], md)[1]).mean()
            assert 0.02 < inv < 0.98, (md, k, inv)
    # partly empty lists beyond the nine planted ones (the scan's fringe): all of them the fallback's, the bound being 3.25 m
    partly = (np.isfinite(md2).sum(1) > 0) & (np.isfinite(md2).sum(1) < 8)
    print("partly empty lists under maxDist 3.25, k = 8:", int(partly.sum()))
    assert partly.sum() >= 50, partly.sum()


def test_query_count_prefixes_mix_both_paths(oracle, brute, pair4k):
    c = far_case(oracle, pair4k, kc.mean_of(kc.partial_reference(pair4k)[0]))
    assert sorted(kc.QUERY_COUNTS) == [1, 63, 64, 65, 255, 256, 257] and kc.QUERY_COUNT_KS == (3, 7)
    assert max(kc.QUERY_COUNTS) <= c["n_far"]
    for k in kc.QUERY_COUNT_KS:
        pairs = [k * nq for nq in kc.QUERY_COUNTS]
        assert min(pairs) < kc.UNPERMUTE_BLOCK < max(pairs)          # k nq on both sides of k_knnk_unpermute's 256 ...
        edge = k * 256                                               # ... and one short of, at and one past a multiple of it
        assert edge % kc.UNPERMUTE_BLOCK == 0 and {edge - k, edge, edge + k} <= set(pairs)
        _ids, bd2 = brute(c["ref_c"], c["q"][:max(kc.QUERY_COUNTS)], k)
        for nq in kc.QUERY_COUNTS[1:]:       # one wave (or few) with lanes of both kinds: a k-th distance above the cap, and
            # one of at most half the cap (the seed's bound is not known here; a ball that small is the tile's as a rule)
            assert kc.necessarily_fallback(bd2[:nq, k - 1]).sum() >= 5 and (bd2[:nq, k - 1] < F(0.5 ** 2)).sum() >= 5, (k, nq)
    assert {63, 64, 65} <= set(kc.QUERY_COUNTS) and kc.TILE_WAVE == 64              # a wave short of, at and past full
    assert {255, 256, 257} <= set(kc.QUERY_COUNTS) and kc.SEED_BLOCK == 256


def test_dense_case_is_one_cell_of_more_than_64_chunks():
    c = dense_case()
    g, ref, cube = c["geom"], c["ref"], c["cube"]
    assert (g["bits"], g["fine"], g["h0"]) == (11, 5, F(kc.DENSE_CELL_SIZE)) and len(ref) <= 8000
    assert len(cube) == kc.DENSE_N > kc.CELL_ROUND * kc.CHUNK_MAX    # more points than 64 chunks hold
    assert len(np.unique(ref[cube, :3], axis=0)) == kc.DENSE_N
    cells, wall = kc.level0_cells(ref, g)
    assert (cells[cube] == np.asarray(kc.DENSE_CELL)).all()          # strictly inside: at least 0.1 m from the cell's walls
    assert wall[cube].min() >= 0.1 - 1e-4, wall[cube].min()
    others = np.delete(np.arange(len(ref)), cube)
    assert not (cells[others] == np.asarray(kc.DENSE_CELL)).all(1).any()
    mid = c["lo"] + kc.DENSE_SIDE / 2
    dist = np.abs(c["q"][:, :3] - mid).max(1) - kc.DENSE_SIDE / 2    # the distance from the cube (queries stand over a face)
    assert (dist[c["group"] == 0] <= 0).all() and np.allclose(dist[c["group"] == 1], 0.5, atol=1e-5)
    assert np.allclose(dist[c["group"] == 2], 5.0, atol=1e-5) and np.bincount(c["group"]).tolist() == [500, 200, 100]


def test_dense_queries_search_the_cube(brute):
    """For every group each of the 8 nearest points is a cube point (the background keeps 11 m off); 5 m away the k-th
    distance is above the cap: the fallback, over the cube's cell at a coarser level; under maxDist 3.25 nothing is in range."""
    c = dense_case()
    ref_c = kc.centred(c["ref"], c["geom"]["mean"])
    ids, d2 = brute(ref_c, kc.centred(c["q"], c["geom"]["mean"]), 8)
    assert np.isin(ids, c["cube"]).all() and (d2[c["group"] < 2, 7] < F(0.9 ** 2)).all()
    assert kc.necessarily_fallback(d2[c["group"] == 2, 0]).all() and (d2[c["group"] == 2, 7] < F(5.5 ** 2)).all()
    assert np.isinf(mask_matches(ids, d2, kc.MAX_DIST_WIDE)[1][c["group"] == 2]).all()


def test_tiny_references_are_distinct_points():
    for k in kc.KS:
        for nr in (k, k + 1):
            ref = kc.tiny_reference(nr)
            assert len(np.unique(ref[:, :3], axis=0)) == nr == len(ref)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", kc.MAX_DISTS, ids=lambda m: "maxdist-%s" % m)
@pytest.mark.parametrize("k", kc.KS)
def test_every_instantiation(handles, oracle, brute, pair4k, k, max_dist):
    ref, at = kc.partial_reference(pair4k)
    h = handles("partial", ref, max_dist)
    c = far_case(oracle, pair4k, h.reference_mean())
    ref_c, q, rows = c["ref_c"], c["q"], c["rows"]
    ids, d2 = h.knn_k(q, k, None)
    bids, bd2 = mask_matches(*brute(ref_c, q, k), max_dist)
    held = check(ids, d2, bids, bd2, ref_c, q)
    print("k", k, "maxDist", max_dist, "necessarily fallback %.3f" % kc.necessarily_fallback(brute(ref_c, q, k)[1][:, -1], max_dist).mean(),
          "invalid entries %.3f" % np.isinf(d2).mean(), "ids held to the brute force's", held, "of", d2.size,
          "differing ids", int((ids != bids).sum()))
    if k == 1 and max_dist is None:                                  # (check() holds knn_k's ids to the rule too, not only d2)
        _i, d1 = h.knn(q, None)
        assert np.array_equal(d1, d2[:, 0])
    if max_dist == kc.MAX_DIST_WIDE:
        for m in kc.CLUSTERS:                                        # m valid entries in ascending order, then -1 / +inf
            r, n = rows[m], min(m, k)
            assert np.array_equal(ids[r, :n], at[m][:n]) and (np.diff(d2[r, :n]) > 0).all() and np.isfinite(d2[r, :n]).all()
            assert (ids[r, n:] == -1).all() and np.isinf(d2[r, n:]).all()
        assert (ids[rows["lonely"]] == -1).all() and np.isinf(d2[rows["lonely"]]).all()
        e = rows["edge"]
        assert bd2[e, 0] == F(10.5625), bd2[e]                       # the construction landed exactly on maxDist ...
        assert d2[e, 0] == F(10.5625) and ids[e, 0] == at[1][0] and (ids[e, 1:] == -1).all()   # ... inclusive: valid


@pytest.mark.gpu
@pytest.mark.parametrize("k,max_dist", [(k, None) for k in kc.KS] + [(k, kc.MAX_DIST_WIDE) for k in (2, 5, 8)])
def test_lattice_ties(handles, brute, k, max_dist):
    c = lattice_case()
    h = handles("lattice", c["ref"], max_dist)
    assert (h.reference_mean() == 0).all()
    ids, d2 = h.knn_k(c["q"], k, None)
    bids, bd2 = mask_matches(*brute(c["ref"], c["q"], k), max_dist)
    held = check(ids, d2, bids, bd2, c["ref"], c["q"])
    print("k", k, "maxDist", max_dist, "differing ids", int((ids != bids).sum()), "held", held, "of", d2.size,
          "invalid entries %.3f" % np.isinf(d2).mean())
    again = h.knn_k(c["q"], k, None)
    assert np.array_equal(again[0], ids) and np.array_equal(again[1], d2)


@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", [None, kc.MAX_DIST_WIDE], ids=lambda m: "maxdist-%s" % m)
def test_lattice_batch_independence(handles, max_dist):
    """The tie rule is a total order on (d2, sorted index): a query's answer cannot depend on its wave neighbours, on the
    level their common box selects, or on whether the tile or the fallback finds it.  64 queries alone (nq = 1), in the batch,
    and in the batch reversed."""
    c = lattice_case()
    q, kind = c["q"], c["kind"]
    h = handles("lattice", c["ref"], max_dist)
    rng = np.random.default_rng(8)
    chosen = np.concatenate([rng.choice(np.flatnonzero(kind == what), 8, replace=False) for what in (kc.CELL, kc.FACE, kc.EDGE, kc.NODE)]
                            + [rng.choice(np.flatnonzero(kind >= kc.OUT_ON), 32, replace=False)])
    assert len(set(chosen.tolist())) == 64
    for k in (2, 5, 8):
        ids, d2 = h.knn_k(q, k, None)
        rids, rd2 = h.knn_k(np.ascontiguousarray(q[::-1]), k, None)
        assert np.array_equal(rids[::-1], ids) and np.array_equal(rd2[::-1], d2), k
        for j in chosen:
            i1, d1 = h.knn_k(q[j:j + 1], k, None)
            assert np.array_equal(i1[0], ids[j]) and np.array_equal(d1[0], d2[j]), (k, j, kc.KIND_NAMES[kind[j]], i1[0], ids[j])


@pytest.mark.gpu
def test_max_dist_beyond_every_answer_changes_nothing(handles):
    """A handle with maxDist 100 m against one without: identical ids and d2 wherever d2 <= 10^4, invalid beyond."""
    c = lattice_case()
    far = kc.points(np.random.default_rng(12).uniform(-100, 100, (300, 3)))
    q = np.concatenate([c["q"], far])
    h0, h100 = handles("lattice", c["ref"], None), handles("lattice", c["ref"], 100.0)
    for k in kc.KS:
        i0, d0 = h0.knn_k(q, k, None)
        i1, d1 = h100.knn_k(q, k, None)
        near = d0 <= F(1e4)
        assert near[:len(c["q"])].all() and 0.2 < near[len(c["q"]):].mean() < 0.8       # both sides of the bound are there
        assert np.array_equal(i1[near], i0[near]) and np.array_equal(d1[near], d0[near]), k
        assert (i1[~near] == -1).all() and np.isinf(d1[~near]).all(), k


def check_copies(ids, bids, n):
    """ids of a reference that holds every point twice (copy i + n of point i), the device's and the brute force's: in the
    device's list the first copy comes first and directly before the second (equal keys: neighbours in the sorted reference)
    and only a first copy stands alone, in the last column; in both lists a second copy has its first before it; and a
    position both lists hold equally often (once: its first copy; twice: both) they hold with the same ids.  (Not column by
    column: within a tie the brute force lists other first copies between a point's two, so one column may hold the device's
    second and the brute force's first copy of one position.)  -> positions compared"""
    second = ids >= n
    assert not second[:, 0].any() and (ids[:, :-1][second[:, 1:]] == ids[:, 1:][second[:, 1:]] - n).all()
    assert not (~second[:, :-1] & (ids[:, 1:] != ids[:, :-1] + n)).any()
    for got in (ids, bids):
        for j, s in zip(*np.nonzero(got >= n)):
            assert got[j, s] - n in got[j, :s], (j, s, got[j])
    compared = 0
    for dev, bru in zip(ids, bids):
        for p in np.intersect1d(dev % n, bru % n):
            d, b = dev[dev % n == p], bru[bru % n == p]
            if len(d) == len(b):
                assert np.array_equal(np.sort(d), np.sort(b)), (dev, bru)
                compared += 1
    assert compared > 0
    return compared


@pytest.mark.gpu
@pytest.mark.parametrize("k", kc.KS)
def test_coincident_points_keep_input_order(handles, brute, k):
    """Every lattice point twice.  Coincident points keep their input order in the sorted reference (the file's docstring), so
    among copies the device's choice is the brute force's: check_copies."""
    c = lattice_case(6, 2)
    ref, q = c["ref"], c["q"]
    h = handles("lattice2", ref, None)
    assert (h.reference_mean() == 0).all()
    ids, d2 = h.knn_k(q, k, None)
    bids, bd2 = brute(ref, q, k)
    check(ids, d2, bids, bd2, ref, q)
    check_copies(ids, bids, len(ref) // 2)


_full = {}


@pytest.mark.gpu
@pytest.mark.parametrize("k", kc.QUERY_COUNT_KS)
@pytest.mark.parametrize("nq", kc.QUERY_COUNTS)
def test_query_counts(handles, oracle, brute, pair4k, nq, k):
    ref, _at = kc.partial_reference(pair4k)
    for max_dist in (None, kc.MAX_DIST_WIDE):
        h = handles("partial", ref, max_dist)
        c = far_case(oracle, pair4k, h.reference_mean())
        ref_c, q = c["ref_c"], c["q"]
        if (k, max_dist) not in _full:
            _full[(k, max_dist)] = h.knn_k(q, k, None)
        fids, fd2 = _full[(k, max_dist)]
        ids, d2 = h.knn_k(q[:nq], k, None)
        assert ids.shape == (nq, k)
        check(ids, d2, *mask_matches(*brute(ref_c, q[:nq], k), max_dist), ref_c, q[:nq])
        assert np.array_equal(ids, fids[:nq]) and np.array_equal(d2, fd2[:nq]), (nq, k, max_dist)


@pytest.mark.gpu
@pytest.mark.parametrize("k", kc.KS)
def test_references_of_k_and_k_plus_one_points(icp_mod, brute, k):
    """nr = k: every list is the whole reference; nr = k + 1: all but the farthest point; ascending both times.  (Fewer than
    k points are refused: test_knn_k_refuses_small_references_and_bad_k.)"""
    q0 = kc.tiny_queries()
    for max_dist in (None, kc.MAX_DIST_WIDE):
        with icp_mod.IcpHandle(matcher_max_dist=max_dist) as h:
            for nr in (k, k + 1):
                ref = kc.tiny_reference(nr)
                h.set_reference(ref, None)
                ref_c = kc.centred(ref, h.reference_mean())
                q = kc.centred(q0, h.reference_mean())
                ids, d2 = h.knn_k(q, k, None)
                wids, wd2 = brute(ref_c, q, k + 1)
                assert (np.diff(wd2[:, :nr], axis=1) > 0).all()      # (distinct distances: the brute force's order is THE order)
                bids, bd2 = mask_matches(wids[:, :k], wd2[:, :k], max_dist)
                check(ids, d2, bids, bd2, ref_c, q)
                assert np.array_equal(ids, bids)
                if max_dist is None:
                    assert np.array_equal(np.sort(ids, axis=1), np.sort(wids[:, :k], axis=1))
                    if nr == k:
                        assert (np.sort(ids, axis=1) == np.arange(k)).all() and (wids[:, k] == -1).all()
                    else:
                        assert ((ids != wids[:, k:]).all(1)).all()   # the farthest point is the one left out
                else:
                    assert 0.02 < np.isinf(d2).mean() < 0.98


@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", [None, kc.MAX_DIST_WIDE], ids=lambda m: "maxdist-%s" % m)
@pytest.mark.parametrize("k", (1, 4, 8))
def test_dense_cell(handles, brute, k, max_dist):
    c = dense_case()
    h = handles("dense", c["ref"], max_dist, kc.DENSE_CELL_SIZE)
    info, g = h.info(), c["geom"]
    assert (info.bits_per_axis, info.fine_bits, F(info.cell_size)) == (g["bits"], g["fine"], g["h0"])
    assert info.n_chunks > kc.CELL_ROUND + 1
    mean = h.reference_mean()
    assert (np.abs(mean - g["mean"]) <= np.spacing(np.abs(g["mean"]))).all()
    ref_c, q = kc.centred(c["ref"], mean), kc.centred(c["q"], mean)
    ids, d2 = h.knn_k(q, k, None)
    wids, wd2 = brute(ref_c, q, k)
    bids, bd2 = mask_matches(wids, wd2, max_dist)
    check(ids, d2, bids, bd2, ref_c, q)
    print("k", k, "maxDist", max_dist, "chunks", info.n_chunks, "invalid entries %.3f" % np.isinf(d2).mean(),
          "necessarily fallback %.3f" % kc.necessarily_fallback(wd2[:, -1], max_dist).mean())
