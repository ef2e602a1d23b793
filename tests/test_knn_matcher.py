"""KDTreeMatcher with knn = k > 1 (k nearest matches) through every layer: both YAML loaders, the config field, and on the
GPU the k-best search (lsgpu_knn_k) against an exact CPU k-NN and the device loop against a test-side loop built from the
oracle's primitives (transform, trimmed limit over all k N distances, point-to-plane on the flattened pairs) and the host
point-to-point solve.

The contract (include/lsgpu_icp.h, matcher_knn): k matches per reading point in ascending d2; TrimmedDistOutlierFilter
ranks all k N distances; every pair with d2 <= limit has weight 1; n_used counts pairs."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from host_loop import build_brute, d2_f32, host_kmatch_icp
from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNN_YAML = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
            "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
            "matcher:\n  KDTreeMatcher:\n    knn: 3\n    epsilon: 0\n"
            "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"
            "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
            "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
            "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
            "      smoothLength: 4\n")


def _with_knn(y, knn, eps="0"):
    return y.replace("    knn: 3\n    epsilon: 0\n", f"    knn: {knn}\n    epsilon: {eps}\n")


# ------------------------------------------------------------------------------------------------ the exact CPU k-NN

@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    """knn_brute (tests/cpp/knn_brute.c): exact k-NN in the device's arithmetic, 16 threads at most."""
    return build_brute(tmp_path_factory.mktemp("knn_brute"))


# ------------------------------------------------------------------------------------------------ CPU: loaders, config

def test_python_loader_accepts_knn():
    from laser_slam_amd import icp
    o = icp.ICP()
    for mini in ("PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer"):
        y = KNN_YAML.replace("PointToPlaneErrorMinimizer", mini)
        for k in (1, 2, 3, 8):
            o.load_from_yaml(io.StringIO(_with_knn(y, k)))
            assert o.chain.matcher_knn == k and o.chain.error_minimizer == mini
        for bad in (_with_knn(y, 0), _with_knn(y, _lib.MATCHER_KNN_MAX + 1), _with_knn(y, 3, "0.1")):
            with pytest.raises(_lib.LsgpuError) as e:
                o.load_from_yaml(io.StringIO(bad))
            assert e.value.code == _lib.BAD_CONFIG and str(_lib.MATCHER_KNN_MAX) in str(e.value)
    # the required modules are still required: a bare k-match matcher is refused for what it lacks
    with pytest.raises(_lib.LsgpuError) as e:
        o.load_from_yaml("matcher:\n  KDTreeMatcher: {knn: 3}\n")
    assert e.value.code == _lib.BAD_CONFIG and "required" in str(e.value)
    assert icp.ChainConfig().matcher_knn == 1


def test_cpp_loader_accepts_knn(tmp_path):
    exe = str(tmp_path / "knn_loader_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "knn_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp",
                           "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "knn_loader_check: ok" in r.stdout, r.stdout + r.stderr


def test_matcher_knn_keeps_the_config_layout():
    c = _lib.IcpConfig()
    assert C.sizeof(c) == 7 * 4 + 8 * 4                        # the struct did not grow
    assert _lib.IcpConfig.reserved.offset == 7 * 4
    assert _lib.IcpConfig.error_minimizer.offset == _lib.IcpConfig.reserved.offset + 4
    assert _lib.IcpConfig.matcher_knn.offset == _lib.IcpConfig.error_minimizer.offset + 4   # today's reserved_[0]
    _lib.lib().lsgpu_icp_config_yaml(C.byref(c))
    assert c.matcher_knn == 0                                  # zero-filled / preset configs: one neighbour
    for bad in (-1, _lib.MATCHER_KNN_MAX + 1, 100):
        c.matcher_knn = bad
        h = C.c_void_p()
        assert _lib.lib().lsgpu_icp_create(C.byref(c), 0, C.byref(h)) == _lib.BAD_CONFIG


def test_brute_helper_is_the_oracle_nearest_neighbour(oracle, brute, pair4k):
    ref, rd = pair4k["ref"], pair4k["rd"]
    ids, d2 = brute(ref, rd, 1)
    oid, od2 = oracle.brute_nn(ref, rd)
    assert np.array_equal(d2[:, 0], od2)
    assert (ids[:, 0] == oid).mean() > 0.999                   # (exact ties may pick another point at the same d2)
    ids3, d23 = brute(ref, rd, 3)
    assert np.array_equal(d23[:, 0], od2) and (np.diff(d23, axis=1) >= 0).all()


# ------------------------------------------------------------------------------------------------ the test-side loop

# host_kmatch_icp and its helpers (_mul4, _p2p_sums, _Cfg) live in tests/host_loop.py


def test_host_loop_with_one_match_is_the_oracle_loop(oracle, brute, pair4k):
    rf, rn = oracle.sampling_surface_normal(pair4k["ref"], 10, 1.0, 0)
    rc, To, sto, tro = oracle.icp_compute(oracle.config_yaml(accum_double=1), pair4k["rd"], rf, rn,
                                          synth.colmajor(pair4k["T_init"]), 40)
    assert rc == 0
    T, it, conv, tr = host_kmatch_icp(oracle, brute, pair4k["rd"], rf, rn, pair4k["T_init"], 1)
    assert (it, int(conv)) == (sto.iterations, sto.converged)
    assert tr == [(np.float32(t["limit"]), int(t["n_used"])) for t in tro]
    assert np.array_equal(T, synth.from_colmajor(To).astype(np.float32))


def test_host_loop_with_three_matches_improves_on_the_guess(oracle, brute, pair64k):
    rf, rn = oracle.sampling_surface_normal(pair64k["ref"], 10, 0.5, 4)
    keep = oracle.random_sampling(len(pair64k["rd"]), 0.5, -1)
    T, it, conv, tr = host_kmatch_icp(oracle, brute, pair64k["rd"][keep], rf, rn, pair64k["T_init"], 3)
    e0 = synth.pose_error(pair64k["T_init"], pair64k["T_true"])
    e1 = synth.pose_error(T.astype(np.float64), pair64k["T_true"])
    assert 1 < it < 40 and e1[0] < e0[0] and e1[1] < e0[1], (e0, e1, it, conv)
    n_reading = len(keep)
    assert all(0 < used <= 3 * n_reading for _lim, used in tr)


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


def _check_knn_k(ids, d2, bids, bd2, ref_c, q):
    """Device k-NN against the exact CPU k-NN of queries q in the centred reference ref_c: ascending, d2 bit for bit,
    ids equal up to exact ties."""
    assert (np.diff(d2, axis=1) >= 0).all()
    assert np.array_equal(d2, bd2)
    # a different id only where the distance is tied: with another match of the query, or at the k-th distance (a point
    # outside the list may be at exactly that distance; the device keeps the smaller Morton index, the helper the smaller
    # input index) -- and the point the device names must lie at exactly the distance it reports, in every column
    ref_c, q = np.ascontiguousarray(ref_c, np.float32), np.ascontiguousarray(q, np.float32)
    jj, ss = np.nonzero(ids != bids)
    for j, s in zip(jj, ss):
        tied = (d2[j] == d2[j, s]).sum() >= 2 or s == d2.shape[1] - 1
        assert tied, (j, s, ids[j], bids[j], d2[j])
    if jj.size:
        assert (ids[jj, ss] >= 0).all() and (ids[jj, ss] < len(ref_c)).all()
        at = d2_f32(q[jj, :3], ref_c[ids[jj, ss], :3])
        bad = np.flatnonzero(at.view(np.uint32) != d2[jj, ss].view(np.uint32))
        assert bad.size == 0, (jj[bad][:5], ss[bad][:5], ids[jj, ss][bad][:5], at[bad][:5], d2[jj, ss][bad][:5])
    # and no point twice in a query's list
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()


@pytest.mark.gpu
def test_knn_k_matches_exact_knn_4k(icp_mod, oracle, brute, pair4k):
    ref, rd = pair4k["ref"], pair4k["rd"]
    with icp_mod.IcpHandle() as h:
        h.set_reference(ref, None)
        mean = h.reference_mean()
        ref_c = ref.copy()
        ref_c[:, :3] -= mean
        T = synth.colmajor(pair4k["T_init"]).copy()
        T[12:15] -= mean
        q = oracle.transform_points(T, rd)
        for k in (2, 3, 8):
            ids, d2 = h.knn_k(rd, k, T)
            bids, bd2 = brute(ref_c, q, k)
            _check_knn_k(ids, d2, bids, bd2, ref_c, q)
        # k = 1 through the same entry point: the distances of lsgpu_knn
        _ids1, d21 = h.knn_k(rd, 1, T)
        _id0, d0 = h.knn(rd, T)
        assert np.array_equal(d21[:, 0], d0)


@pytest.mark.gpu
def test_knn_k_matches_exact_knn_full_size_sample(icp_mod, oracle, brute):
    ref, rd, _T_true, T_init = synth.scan_pair(16384)
    sample = np.random.default_rng(20).choice(len(rd), 20000, replace=False)
    with icp_mod.IcpHandle() as h:
        h.set_reference(ref, None)
        mean = h.reference_mean()
        ref_c = ref.copy()
        ref_c[:, :3] -= mean
        T = synth.colmajor(T_init).copy()
        T[12:15] -= mean
        ids, d2 = h.knn_k(rd[sample], 3, T)
    q = oracle.transform_points(T, rd[sample])
    bids, bd2 = brute(ref_c, q, 3)
    _check_knn_k(ids, d2, bids, bd2, ref_c, q)


@pytest.mark.gpu
def test_knn_k_refuses_small_references_and_bad_k(icp_mod, pair4k):
    with icp_mod.IcpHandle() as h:
        h.set_reference(pair4k["ref"][:5], None)
        for k in (6, 0, _lib.MATCHER_KNN_MAX + 1):
            with pytest.raises(_lib.LsgpuError) as e:
                h.knn_k(pair4k["rd"], k)
            assert e.value.code == _lib.BAD_ARG
    with icp_mod.IcpHandle(matcher_knn=8) as h:
        h.set_reference(pair4k["ref"][:7], pair4k["ref"][:7, :3] * 0 + np.float32([0, 0, 1]))
        with pytest.raises(_lib.LsgpuError) as e:
            h.align(pair4k["rd"], pair4k["T_init"])
        assert e.value.code == _lib.BAD_ARG and "fewer points" in str(e.value)


def _device_vs_host(icp_mod, oracle, brute, pair, k, p2p, seed=4):
    ref, rd, T_init = pair["ref"], pair["rd"], pair["T_init"]
    rf, rn = oracle.sampling_surface_normal(ref, 10, 0.5, seed)
    keep = oracle.random_sampling(len(rd), 0.5, -1)
    mini = "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer"
    with icp_mod.IcpHandle(None, 0, mini, matcher_knn=k) as h:
        h.set_reference(rf, None if p2p else rn)
        Tg, st = h.align(rd[keep], T_init)
        trg = [(np.float32(t["limit"]), int(t["n_used"])) for t in h.trace()]
        mean = h.reference_mean()
    Th, ith, convh, trh = host_kmatch_icp(oracle, brute, rd[keep], rf, rn, T_init, k, p2p=p2p, mean=mean)
    return Tg, st, trg, Th, ith, convh, trh


@pytest.mark.gpu
@pytest.mark.parametrize("k,p2p", [(3, False), (3, True), (8, False), (2, False), (5, False), (6, True), (7, False)])
def test_device_loop_matches_host_loop_4k(icp_mod, oracle, brute, pair4k, k, p2p):
    Tg, st, trg, Th, ith, convh, trh = _device_vs_host(icp_mod, oracle, brute, pair4k, k, p2p)
    assert (st.iterations, st.converged) == (ith, int(convh)), (st.iterations, st.converged, ith, convh)
    assert trg == trh
    assert st.final_n_used == trh[-1][1]
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    assert dt <= 1e-5 and dr <= 1e-6, (dt, dr)


@pytest.mark.gpu
def test_device_loop_matches_host_loop_64k(icp_mod, oracle, brute, pair64k):
    Tg, st, trg, Th, ith, convh, trh = _device_vs_host(icp_mod, oracle, brute, pair64k, 3, False)
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    assert dt <= 1e-4 and dr <= 1e-5, (dt, dr, st.iterations, ith)


@pytest.mark.gpu
def test_full_size_pair_converges_with_three_matches(icp_mod):
    ref, rd, T_true, T_init = synth.scan_pair(16384)
    with icp_mod.IcpHandle(None, 0, "PointToPointErrorMinimizer", matcher_knn=3) as h:
        T, st = h.compute(rd, ref, T_init, 0.5, 0, 0.5, seed=5)
    e0 = synth.pose_error(T_init, T_true)
    e1 = synth.pose_error(T.astype(np.float64), T_true)
    assert 1 < st.iterations <= 40 and e1[0] < e0[0] and e1[1] < e0[1], (e0, e1, st.iterations)
    # about ratio x 3 x N pairs (the reading filter keeps about half of the points)
    want = 0.75 * 3 * 0.5 * len(rd)
    assert abs(st.final_n_used - want) < 0.02 * want, (st.final_n_used, want)


@pytest.mark.gpu
def test_align_batch_with_three_matches_is_sequential_align(icp_mod, oracle):
    pairs = []
    for i, n_az in enumerate([96, 160, 64, 128]):
        ref, rd, _Tt, Ti = synth.scan_pair(n_az, noise_seeds=(3000 + i, 4000 + i), guess_seed=3000 + i)
        rf, rn = oracle.sampling_surface_normal(ref, 10, 0.5, i)
        pairs.append((rf, rn, rd, Ti))
    refs, nrms, rds, Tis = map(list, zip(*pairs))
    hs = [icp_mod.IcpHandle(matcher_knn=3) for _ in range(2)]
    Tb, stb, rcb = icp_mod.align_batch(hs, refs, nrms, rds, Tis)
    for h in hs:
        h.close()
    assert list(rcb) == [0] * len(pairs)
    with icp_mod.IcpHandle(matcher_knn=3) as h:
        for i, (rf, rn, rd, Ti) in enumerate(pairs):
            h.set_reference(rf, rn)
            T, st = h.align(rd, Ti)
            assert np.array_equal(T, Tb[i]) and st.iterations == stb[i].iterations and st.iterations > 1


@pytest.mark.gpu
def test_compute_clouds_and_yaml_facade_with_three_matches(icp_mod, pair64k):
    ref, rd, T_init = pair64k["ref"], pair64k["rd"], pair64k["T_init"]
    with icp_mod.IcpHandle(matcher_knn=3) as h:
        Tc, stc = h.compute(rd, ref, T_init, 0.5, 10, 0.5, seed=3)
        h.cloud_upload(0, ref)
        h.cloud_upload(1, rd)
        Tk, stk = h.compute_clouds(1, [0], None, T_init, 0.5, 10, 0.5, seed=3)
    assert stc.iterations == stk.iterations > 1 and np.array_equal(Tc, Tk)
    o = icp_mod.ICP()
    o.load_from_yaml(io.StringIO(KNN_YAML))
    assert o.chain.matcher_knn == 3
    o.chain.seed = 3
    T = o.compute(rd, ref, T_init)
    assert np.array_equal(T, Tc)
    e0 = synth.pose_error(T_init, pair64k["T_true"])
    e1 = synth.pose_error(T.astype(np.float64), pair64k["T_true"])
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)


@pytest.mark.gpu
def test_one_match_handle_is_unaffected_by_a_three_match_handle(icp_mod, pair64k):
    ref, rd, T_init = pair64k["ref"], pair64k["rd"], pair64k["T_init"]
    with icp_mod.IcpHandle() as h1:
        T0, st0 = h1.compute(rd, ref, T_init, 0.5, 10, 0.5, seed=6)
        tr0 = [(t["limit"], t["n_used"]) for t in h1.trace()]
    with icp_mod.IcpHandle() as h1, icp_mod.IcpHandle(matcher_knn=3) as h3:
        T3a, _ = h3.compute(rd, ref, T_init, 0.5, 10, 0.5, seed=7)
        T1, st1 = h1.compute(rd, ref, T_init, 0.5, 10, 0.5, seed=6)
        tr1 = [(t["limit"], t["n_used"]) for t in h1.trace()]
        T3b, _ = h3.compute(rd, ref, T_init, 0.5, 10, 0.5, seed=7)
    assert np.array_equal(T0, T1) and st0.iterations == st1.iterations and tr0 == tr1
    assert np.array_equal(T3a, T3b)


@pytest.mark.gpu
def test_split_scan_refuses_a_k_match_handle(icp_mod, pair4k):
    with icp_mod.IcpHandle(matcher_knn=3) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, icp_mod.comm_unique_id())
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value)
        h.set_reference(pair4k["ref"], None)                   # the handle stays usable on its own
        ids, d2 = h.knn_k(pair4k["rd"], 3)
        assert ids.shape == (len(pair4k["rd"]), 3)
