"""The align loop's last kernel (k_normal_eq_loop) and the stand-alone sums (k_normal_eq, k_ne_final) across reading sizes:
every grid, unroll slot and shape of the last block's reduction that depends on nothing but the count
(tests/size_cases.py has the sizes, what each reaches, and the numpy model of one iteration's sums).

CPU part (no marker): the cases' conditions -- grid, unroll slot and rounds as the list claims, the oracle converges in
more than 4 iterations from 63 points on and not at 7 -- and the model against the oracle's own trace: limit bit for bit,
n_used exactly, A and b per entry within 1e-12 of sum |term|.

Device part: per size two alignments on one handle -- iteration count, converged, per iteration the limit bit for bit and
n_used against the oracle; A and b per entry within 1e-12 of sum |term| of the model fed the device's own pose (the bar is
derived: at most about 80 dependent double additions, 80 x 2^-53 = 1e-14, x 100; the model's sum is exact); the pose within
1e-4 m / 1e-5 rad of the oracle's; both alignments the same bytes.  The same through tests/size_worker.py with
LSGPU_NE_BLOCKS=64 (one process; a worker that dies, faults or overruns its time limit fails its test and nothing further is
started on the device: the remaining device tests skip, naming it).  Point-to-point and knn = 3 against the test-side loop
of tests/host_loop.py; align_batch over four sizes at once; lsgpu_normal_eq / lsgpu_point_to_point with invalid ids,
NaN and +inf distances, a limit that keeps nothing and a limit of +inf.

Seen on an MI355X (every test prints its figures, -s): worst |device - model| / sum |term| over all sizes and iterations
3.6e-16 for A and 2.0e-16 for b at the default block count, 2.8e-16 / 1.8e-16 with 64 blocks, 4.2e-16 (point-to-plane) and
3.0e-16 (point-to-point) for the stand-alone sums; no tied kept pair anywhere; every pose equal to the oracle's / the host
loop's bit for bit.

Wall time on an MI355X: 7.8 s for the file's device part -- 3.8 s of it the worker (1.6 s in its five checked sizes, the rest
interpreter start, library load and the scans), 2.2 s the first handle and the scans, under 0.3 s per other test; about 3 s
for its CPU part on eight cores.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import host_loop
import size_cases as sz
from laser_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER_TIMEOUT = 120    # s (tests/test_select_paths.py's): interpreter start, library load, two scans and five checked sizes
CONVERGING = [n for n in sz.DEFAULT_SIZES if n >= 63]


@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    return host_loop.build_brute(tmp_path_factory.mktemp("knn_brute"))


@pytest.fixture(scope="module")
def cpu_model(oracle, brute):
    return sz.Model(oracle, brute, *sz.reference(oracle))


# ------------------------------------------------------------------------------------------------ the cases, on the CPU
def test_sizes_reach_what_the_list_claims(oracle):
    rf, rn = sz.reference(oracle)
    assert rf.shape == (2026, 4) and rn.shape == (2026, 3)
    assert len(sz.scans(sz.RD_AZ)[1]) == 69461 >= max(sz.DEFAULT_SIZES)
    for sizes, blocks in ((sz.DEFAULT_SIZES, sz.DEFAULT_BLOCKS), (sz.WORKER_SIZES, sz.WORKER_BLOCKS)):
        for n, (nb, slot, rounds, _why) in sizes.items():
            assert nb == min(blocks, -(-n // 256)), n
            assert (n > 256 * nb) == (slot >= 1) and (n > 8 * 256 * nb) == (rounds == 2), n
            assert sz.grid(n, blocks) == (nb, slot, rounds), (n, sz.grid(n, blocks))
    for n, nb in sz.KNN3_SIZES.items():
        assert sz.grid(3 * n)[0] == nb, n
    # the shapes of the last block's reduction the sizes are there for
    shape = {n: sz.tail_shape(v[0]) for n, v in sz.DEFAULT_SIZES.items()}
    assert shape[255]["filled"] == 1 and shape[257]["filled"] == 2
    assert shape[1793] == dict(per=1, filled=8, past_end=0, batches=0, singles=1)
    assert shape[2049] == dict(per=2, filled=5, past_end=3, batches=0, singles=2)
    assert shape[30720] == dict(per=15, filled=8, past_end=0, batches=0, singles=15)
    assert shape[30721] == dict(per=16, filled=8, past_end=0, batches=1, singles=9)
    assert shape[32769] == dict(per=17, filled=8, past_end=0, batches=1, singles=10)
    assert shape[65281] == shape[65537] == dict(per=32, filled=8, past_end=0, batches=2, singles=0)
    assert sz.tail_shape(64) == dict(per=8, filled=8, past_end=0, batches=0, singles=8)


@pytest.mark.parametrize("n", list(sz.DEFAULT_SIZES))
def test_oracle_converges_from_63_points_on(oracle, n):
    r = sz.oracle_run(oracle, n)
    if n < 63:
        assert r["rc"] == 1, (n, r["rc"])            # NO_CONVERGENCE
        return
    assert r["rc"] == 0 and r["converged"] == 1 and 4 < r["iterations"] == len(r["trace"]) < 40, (n, r["rc"], r["iterations"])


@pytest.mark.parametrize("n", CONVERGING)
def test_model_reproduces_the_oracles_trace(oracle, cpu_model, n):
    r = sz.oracle_run(oracle, n)
    out = cpu_model.check_trace(cpu_model.moved(sz.reading(n), sz.poses()[0]), r["trace"])
    print("n", n, "iterations", r["iterations"], "worst |oracle - model| / sum |term|: A", out["worst_A"], "b", out["worst_b"],
          "tied kept pairs", out["ties"])
    assert not out["failures"], (n, out["failures"][:8])


# ------------------------------------------------------------------------------------------------ the device runs
_STOPPED = None     # why nothing further is started on the device
_DEFAULT = {}       # size -> device_case's facts at the default block count


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
def dev(oracle, brute):
    """One point-to-plane, 1-NN handle with the reference set once, and the model on that handle's reference mean."""
    from laser_slam_amd import icp
    rf, rn = sz.reference(oracle)
    with icp.IcpHandle() as h:
        h.set_reference(rf, rn)
        mean = h.reference_mean()
        assert np.array_equal(mean, sz.reference_mean(rf))
        yield h, sz.Model(oracle, brute, rf, rn, mean)


def _default_case(oracle, dev, n):
    if n not in _DEFAULT:
        h, model = dev
        _DEFAULT[n] = _guard(lambda: sz.device_case(oracle, model, h, n), f"the alignment of {n} points")
    return _DEFAULT[n]


def _report(tag, n, blocks, c):
    nb, slot, rounds = sz.grid(n, blocks)
    print(tag, "n", n, "grid", nb, sz.tail_shape(nb), "highest unroll slot", slot, "rounds", rounds, "iterations", c["iterations"],
          "worst |device - model| / sum |term|: A", c["worst_A"], "b", c["worst_b"], "tied kept pairs", c["ties"],
          "pose vs oracle", c["dt"], "m", c["dr"], "rad")


@pytest.mark.gpu
@pytest.mark.parametrize("n", CONVERGING)
def test_point_to_plane_sums_at_every_size(oracle, dev, n):
    _device_or_skip()
    c = _default_case(oracle, dev, n)
    _report("default", n, sz.DEFAULT_BLOCKS, c)
    assert not c["failures"], (n, c["failures"][:8])
    assert c["ties"] <= sz.TIE_CAP


@pytest.mark.gpu
def test_seven_points_do_not_converge(oracle, dev):
    _device_or_skip()
    from laser_slam_amd._lib import ConvergenceError
    assert sz.oracle_run(oracle, 7)["rc"] == 1
    h, model = dev
    before = _default_case(oracle, dev, 63)
    for _ in range(2):
        with pytest.raises(ConvergenceError):
            _guard(lambda: h.align(sz.reading(7), sz.poses()[0]), "the alignment of 7 points")
    after = _guard(lambda: sz.device_case(oracle, model, h, 63), "the alignment of 63 points")     # the handle is as good as before
    assert not after["failures"] and after["digest"] == before["digest"], after["failures"][:8]


def _host_case(icp_mod, oracle, brute, n, k, p2p):
    """The device loop and the test-side loop on the reading of n points -> what test_device_loop_matches_host_loop_4k
    compares."""
    rf, rn = sz.reference(oracle)
    rd, T_init = sz.reading(n), sz.poses()[0]
    mini = "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer"
    with icp_mod.IcpHandle(None, 0, mini, matcher_knn=k) as h:
        h.set_reference(rf, None if p2p else rn)
        Tg, st = _guard(lambda: h.align(rd, T_init), f"the alignment of {n} points, k {k}, {mini}")
        trg = h.trace()
        mean = h.reference_mean()
    search, tree = brute, []
    if k == 1:      # the oracle's k-d tree behind the helper's interface (the loop centres the reference once)
        def search(ref_c, q, _k):
            if not tree:
                tree.append(oracle.KdTree(ref_c))
            ids, d2 = tree[0].nn(q, threads=16)
            return ids[:, None], d2[:, None]
    Th, ith, convh, trh = host_loop.host_kmatch_icp(oracle, search, rd, rf, rn, T_init, k, p2p=p2p, mean=mean)
    return Tg, st, trg, Th, ith, convh, trh


def _assert_host_case(case, label):
    Tg, st, trg, Th, ith, convh, trh = case
    got = [(np.float32(t["limit"]), int(t["n_used"])) for t in trg]
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    print(label, "iterations", st.iterations, "pose vs the host loop", dt, "m", dr, "rad")
    assert (st.iterations, st.converged) == (ith, int(convh)), (label, st.iterations, st.converged, ith, convh)
    assert got == trh, (label, [k for k, (a, b) in enumerate(zip(got, trh)) if a != b])
    assert st.final_n_used == trh[-1][1]
    assert dt <= 1e-5 and dr <= 1e-6, (label, dt, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("n", sz.P2P_SIZES)
def test_point_to_point_loop_at_every_size(oracle, brute, n):
    _device_or_skip()
    from laser_slam_amd import icp
    _assert_host_case(_host_case(icp, oracle, brute, n, 1, True), f"point-to-point n {n} grid {sz.grid(n)[0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", list(sz.KNN3_SIZES))
def test_three_match_loop_at_every_size(oracle, brute, n):
    _device_or_skip()
    from laser_slam_amd import icp
    _assert_host_case(_host_case(icp, oracle, brute, n, 3, False), f"knn 3 n {n} grid {sz.grid(3 * n)[0]}")


@pytest.mark.gpu
@pytest.mark.timeout(180)
def test_another_block_count(oracle, dev):
    """LSGPU_NE_BLOCKS=64 in a process of its own: unroll slots 1-7, the second round of the outer loop, the grids 9 and
    64.  2049 points have grid 9 under either count -- the same bytes as here; 30 721 have 121 blocks here and 64 there --
    another order of the same sum, which shows that the worker really ran with the other count."""
    global _STOPPED
    _device_or_skip()
    env = dict(os.environ)
    env["LSGPU_NE_BLOCKS"] = str(sz.WORKER_BLOCKS)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "size_worker.py")]
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    except subprocess.TimeoutExpired:
        _STOPPED = f"the size worker overran its {WORKER_TIMEOUT} s"
        pytest.fail(_STOPPED)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("SIZE_RESULT ")]
    if p.returncode != 0 or not line:
        _STOPPED = f"the size worker ended with status {p.returncode}"
        pytest.fail(f"{_STOPPED}\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
    res = json.loads(line[0][len("SIZE_RESULT "):])
    hip = [n for n, c in res["cases"].items() if c.get("code") == 3]
    if hip:
        _STOPPED = f"a HIP error in the size worker, {hip[0]} points"
        pytest.fail(f"{_STOPPED}: {res['cases'][hip[0]]}")
    print("worker: %.2f s" % res["seconds"], "blocks", res["blocks"], "points of the dense reading", res["big_reading"])
    assert res["blocks"] == str(sz.WORKER_BLOCKS) and res["big_reading"] >= max(sz.WORKER_SIZES)
    assert sorted(res["cases"], key=int) == [str(n) for n in sorted(sz.WORKER_SIZES)], sorted(res["cases"])
    for n in sz.WORKER_SIZES:
        c = res["cases"][str(n)]
        assert "error" not in c, (n, c)
        _report("worker", n, sz.WORKER_BLOCKS, c)
        assert not c["failures"], (n, c["failures"][:8])
        assert c["ties"] <= sz.TIE_CAP
    assert res["cases"]["2049"]["digest"] == _default_case(oracle, dev, 2049)["digest"]
    assert res["cases"]["30721"]["digest"] != _default_case(oracle, dev, 30721)["digest"]


@pytest.mark.gpu
def test_align_batch_over_mixed_sizes(oracle, dev):
    """test_align_batch_matches_sequential varies the pool, the references and readings of 4-13 k points;
    test_align_batch_reuses_a_shared_reference shares one reference among readings of one size.  Here: one shared
    reference, readings of 63 to 30 721 points side by side -- grids 1, 2, 9 and 121 in flight together -- and the whole
    trace, not the pose alone."""
    _device_or_skip()
    from laser_slam_amd import icp
    rf, rn = sz.reference(oracle)
    T_init = sz.poses()[0]
    rds = [sz.reading(n) for n in sz.BATCH_SIZES]
    B = len(rds)
    hs = [icp.IcpHandle() for _ in range(B)]
    try:
        T, st, rc = _guard(lambda: icp.align_batch(hs, [rf] * B, [rn] * B, rds, [T_init] * B), "align_batch")
        traces = [h.trace() for h in hs]
    finally:
        for h in hs:
            h.close()
    assert list(rc) == [0] * B
    h, _model = dev
    for i, n in enumerate(sz.BATCH_SIZES):
        Ts, sts = _guard(lambda: h.align(rds[i], T_init), f"the alignment of {n} points")
        assert T[i].tobytes() == Ts.tobytes(), n
        assert (st[i].iterations, st[i].converged, st[i].final_n_used) == (sts.iterations, sts.converged, sts.final_n_used), n
        assert sz.trace_bytes(traces[i]) == sz.trace_bytes(h.trace()), n


# ------------------------------------------------------------------------------------------------ the stand-alone sums
@pytest.mark.gpu
@pytest.mark.parametrize("p2p", [False, True], ids=["normal_eq", "point_to_point"])
def test_stand_alone_sums_skip_what_is_invalid(oracle, dev, p2p):
    """lsgpu_normal_eq / lsgpu_point_to_point (k_normal_eq, k_ne_final; the entry points do not look at the handle's
    minimizer) from 1 to 65 537 pairs -- the last with the full grid and a second grid-stride round -- with ids of -1, NaN
    and +inf distances among the matches."""
    _device_or_skip()
    h, model = dev
    T16 = model.mean_frame_pose(sz.poses()[0])
    call = h.point_to_point if p2p else h.normal_eq

    def sums(query, ids, d2, limit):
        out = _guard(lambda: call(query, T16, ids, d2, limit), f"the stand-alone sums of {len(query)} pairs")
        if p2p:
            return out
        A, b, used, r2 = out
        assert np.array_equal(A, A.T)
        return np.concatenate([A[np.triu_indices(6)], b, [used, r2]])

    worst = 0.0
    for nq in sz.SUMS_SIZES:
        query = sz.reading(nq)
        ids, d2 = _guard(lambda: h.knn(query, T16), f"the search of {nq} points")
        rank = min(nq - 1, int(np.float32(nq) * np.float32(sz.RATIO)))
        trim = float(np.partition(d2, rank)[rank])
        fine = d2 <= np.float32(trim)               # what the clean matches keep
        ids[6::7] = -1
        d2[5::11] = np.nan
        d2[3::13] = np.inf
        no_id, nan, inf = ids < 0, np.isnan(d2), np.isinf(d2)
        if nq >= 64:                                # each skip path fires on a pair nothing else rejects, and pairs remain
            assert (no_id & fine & ~nan & ~inf).any() and (nan & fine & ~no_id).any() and (inf & fine & ~no_id).any()
            assert (~fine & ~no_id & ~nan & ~inf).any()
        for limit in (trim, -1.0, float("inf")):
            got = sums(query, ids, d2, limit)
            assert got.tobytes() == sums(query, ids, d2, limit).tobytes(), (nq, limit)
            want, mag, keep = model.sums(query, T16, ids, d2, limit, p2p)
            assert got[27] == want[27] == keep.sum(), (nq, limit, got[27], int(keep.sum()))
            if limit == -1.0:
                assert not keep.any() and not got.any() and not np.signbit(got).any(), (nq, got)
                continue
            if limit == trim:
                assert np.array_equal(keep, fine & ~no_id & ~nan & ~inf) and (nq < 64 or 0 < keep.sum() < nq)
            else:
                assert np.array_equal(keep, ~no_id & ~nan & ~inf) and (nq < 64 or keep.sum() > (fine & keep).sum())
            err = np.abs(got - want)
            ratio = float((err / np.where(mag > 0, mag, 1.0)).max())
            worst = max(worst, ratio)
            print("p2p" if p2p else "plane", "nq", nq, "limit", limit, "kept", int(keep.sum()), "worst |device - model| / sum |term|", ratio)
            assert (err <= sz.BAR * mag).all(), (nq, limit, np.flatnonzero(~(err <= sz.BAR * mag)), ratio)
            if p2p:
                assert not got[15:27].any()
    print("p2p" if p2p else "plane", "worst ratio over all sizes", worst)
