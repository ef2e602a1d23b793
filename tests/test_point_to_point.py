"""PointToPointErrorMinimizer (libpointmatcher's second standard minimizer) through every layer: both YAML loaders,
the host solve lsgpu_point_to_point_solve against numpy's SVD, and on the GPU the device loop against a test-side ICP
loop built from the oracle's primitives (filters, kd-tree, trimmed limit) and the host solve.

The contract (include/lsgpu_icp.h): W = sum w, p_ = sum w p / W, q_ = sum w q / W, M = sum w (q - q_)(p - p_)^T = U S V^T,
R = U V^T (U diag(1,1,-1) V^T if det < 0), t = q_ - R p_, T_iter <- [R t] T_iter; W == 0 -> LSGPU_NO_CONVERGENCE."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P2P_YAML = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
            "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"
            "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n"
            "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"
            "errorMinimizer:\n  PointToPointErrorMinimizer\n"
            "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
            "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
            "      smoothLength: 4\n")


def _without_reference_filter(y):
    return y.replace("referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n", "")


# ------------------------------------------------------------------------------------------------ CPU: the loaders

def test_python_loader_accepts_point_to_point_chains():
    from laser_slam_amd import icp
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(P2P_YAML))
    ch = o.chain
    assert ch.error_minimizer == "PointToPointErrorMinimizer"
    assert (ch.reading_sampling_prob, ch.surface_normal_knn, ch.trim_ratio, ch.max_iterations) == (0.5, 10, 0.75, 40)
    # the normal filter is optional for point-to-point: no module, no normals, the reference as given
    o.load_from_yaml(io.StringIO(_without_reference_filter(P2P_YAML)))
    assert o.chain.error_minimizer == "PointToPointErrorMinimizer" and o.chain.surface_normal_knn == 0
    assert o.chain.trim_ratio == 0.75 and o.chain.reading_sampling_prob == 0.5
    # point-to-plane keeps requiring the normals; every chain keeps requiring a matcher and a counter
    p2pl = P2P_YAML.replace("PointToPointErrorMinimizer", "PointToPlaneErrorMinimizer")
    o.load_from_yaml(io.StringIO(p2pl))
    assert o.chain.error_minimizer == "PointToPlaneErrorMinimizer" and o.chain.surface_normal_knn == 10
    bad = [_without_reference_filter(p2pl),
           P2P_YAML.replace("matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n", ""),
           P2P_YAML.replace("  - CounterTransformationChecker:\n      maxIterationCount: 40\n", ""),
           P2P_YAML.replace("errorMinimizer:\n  PointToPointErrorMinimizer\n", ""),
           "errorMinimizer: PointToPointErrorMinimizer\n",
           P2P_YAML.replace("PointToPointErrorMinimizer", "PointToPointSimilarityErrorMinimizer")]
    for y in bad:
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(y))
        assert e.value.code == _lib.BAD_CONFIG, y


def test_cpp_loader_accepts_point_to_point_chains(tmp_path):
    exe = str(tmp_path / "p2p_loader_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "p2p_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp",
                           "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "p2p_loader_check: ok" in r.stdout, r.stdout + r.stderr


def test_minimizer_field_keeps_the_config_layout():
    c = _lib.IcpConfig()
    assert C.sizeof(c) == 7 * 4 + 8 * 4                        # the struct did not grow
    assert _lib.IcpConfig.error_minimizer.offset == _lib.IcpConfig.reserved.offset + 4   # today's reserved[1]
    _lib.lib().lsgpu_icp_config_yaml(C.byref(c))
    assert c.error_minimizer == _lib.MINIMIZER_POINT_TO_PLANE    # zero-filled / preset configs keep point-to-plane
    for bad in (2, -1, 7):
        c.error_minimizer = bad
        h = C.c_void_p()
        assert _lib.lib().lsgpu_icp_create(C.byref(c), 0, C.byref(h)) == _lib.BAD_CONFIG


# ------------------------------------------------------------------------------------------------ CPU: the solve

def _sums(p, q):
    """The 29 sums of the device kernels, in float64 (p, q: float32 (n, 3))."""
    pd, qd = p.astype(np.float64), q.astype(np.float64)
    e = (p - q).astype(np.float64)
    s = np.zeros(29)
    s[0:3] = pd.sum(0)
    s[3:6] = qd.sum(0)
    s[6:15] = np.einsum("na,nc->ac", qd, pd).ravel()
    s[27] = len(p)
    s[28] = (e * e).sum()
    return s


def _svd_reference(s):
    W = s[27]
    pb, qb = s[0:3] / W, s[3:6] / W
    M = s[6:15].reshape(3, 3) - W * np.outer(qb, pb)
    U, _S, Vt = np.linalg.svd(M)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return R, qb - R @ pb


def _angle(Ra, Rb):
    # |R_a - R_b|_F = 2 sqrt(2) sin(theta / 2): precise for small angles
    return 2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0))))


def _random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_point_to_point_solve_matches_numpy_svd():
    from laser_slam_amd import icp
    rng = np.random.default_rng(2026)
    worst_r = worst_t = 0.0
    for _ in range(1200):
        n = int(rng.integers(8, 400))
        p = (rng.normal(size=(n, 3)) * rng.uniform(0.5, 20.0, size=3)).astype(np.float32)
        R0, t0 = _random_rotation(rng), rng.uniform(-5.0, 5.0, size=3)
        q = (p.astype(np.float64) @ R0.T + t0 + rng.normal(size=(n, 3)) * 0.02).astype(np.float32)
        s = _sums(p, q)
        T = icp.point_to_point_solve(s)
        R, t = _svd_reference(s)
        assert T.dtype == np.float32 and np.array_equal(T[3], [0, 0, 0, 1])
        worst_r = max(worst_r, _angle(T[:3, :3].astype(np.float64), R))
        worst_t = max(worst_t, float(np.abs(T[:3, 3] - t).max()))
    assert worst_r <= 1e-6 and worst_t <= 1e-6, (worst_r, worst_t)


def test_point_to_point_solve_reflection_and_degenerate_cases():
    from laser_slam_amd import icp
    rng = np.random.default_rng(7)
    # det(U V^T) < 0: the reading is a mirror image of the reference (distinct singular values, so the best proper
    # rotation is unique: U diag(1,1,-1) V^T)
    for _ in range(50):
        p = (rng.normal(size=(200, 3)) * [9.0, 4.0, 1.5]).astype(np.float32)
        Rm = _random_rotation(rng) @ np.diag([1.0, 1.0, -1.0])
        q = (p.astype(np.float64) @ Rm.T + rng.uniform(-3, 3, 3)).astype(np.float32)
        s = _sums(p, q)
        W = s[27]
        M = s[6:15].reshape(3, 3) - np.outer(s[3:6], s[0:3]) / W
        U, _S, Vt = np.linalg.svd(M)
        assert np.linalg.det(U @ Vt) < 0
        T = icp.point_to_point_solve(s)
        R, t = _svd_reference(s)
        Rg = T[:3, :3].astype(np.float64)
        assert abs(np.linalg.det(Rg) - 1.0) < 1e-5
        assert _angle(Rg, R) <= 1e-6 and np.abs(T[:3, 3] - t).max() <= 1e-6
    # no pair: ConvergenceError ("no point to minimize"), the C entry point returns NO_CONVERGENCE
    with pytest.raises(_lib.ConvergenceError):
        icp.point_to_point_solve(np.zeros(29))
    out = np.zeros(16, np.float32)
    z = np.zeros(29)
    assert _lib.lib().lsgpu_point_to_point_solve(z.ctypes.data_as(C.POINTER(C.c_double)),
                                                 out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.NO_CONVERGENCE
    # rank-deficient M: collinear matches (rank 1), coincident matches (rank 0), one pair
    line = np.outer(np.linspace(-5, 5, 50), [0.3, -0.8, 0.5]).astype(np.float32)
    cases = [(line, (line.astype(np.float64) @ _random_rotation(rng).T + 1.0).astype(np.float32)),
             (np.tile(np.float32([[1, 2, 3]]), (10, 1)), np.tile(np.float32([[4, 5, 6]]), (10, 1))),
             (np.float32([[1, 2, 3]]), np.float32([[-1, 0, 2]]))]
    for p, q in cases:
        T = icp.point_to_point_solve(_sums(p, q))
        R = T[:3, :3].astype(np.float64)
        assert np.isfinite(T).all()
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R) - 1.0) < 1e-5
        # whatever rotation the degenerate case picks, the centroids are matched
        pb, qb = p.astype(np.float64).mean(0), q.astype(np.float64).mean(0)
        assert np.abs(R @ pb + T[:3, 3] - qb).max() < 1e-4


# ------------------------------------------------------------------------------------------------ the test-side loop

def _mul4(a, b):
    """a @ b in float32 with the operation order of hostmath::mul4 (4x4, row-major numpy)."""
    s = a[:, 0:1] * b[0:1, :]
    s = s + a[:, 1:2] * b[1:2, :]
    s = s + a[:, 2:3] * b[2:3, :]
    s = s + a[:, 3:4] * b[3:4, :]
    return s.astype(np.float32)


def _rotation_distance(Ta, Tb):
    from laser_slam_amd import icp
    return np.float32(icp.rotation_distance(Ta, Tb))


def host_p2p_icp(oracle, rd, ref, T_init, cfg):
    """ICP::compute steps 2-7 with PointToPointErrorMinimizer: centre the reference on its mean,
    move the reading by T_refMean_dataIn, then {transform, 1-NN, trimmed limit, point-to-point step, checkers}.  Every
    transform is oracle.transform_points, so the queries carry the device's bits.  -> (T 4x4 float32, iterations,
    converged, [(limit, n_used)])."""
    from laser_slam_amd import icp
    mean = (ref[:, :3].astype(np.float64).sum(0) / len(ref)).astype(np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T_rm_in = np.asarray(T_init, np.float32).copy()
    T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
    reading = oracle.transform_points(synth.colmajor(T_rm_in), rd)
    tree = oracle.KdTree(ref_c)
    T_iter = np.eye(4, dtype=np.float32)
    hist = [T_iter.copy()]                        # checkers.init(T_iter)
    rot7 = [np.float32(0)]
    counter, it, converged, trace = 0, 0, False, []
    smooth = cfg.smooth_length
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = tree.nn(step, threads=16)
        rc, limit = oracle.trim_limit(d2, cfg.trim_ratio)
        assert rc == 0
        w = d2 <= np.float32(limit)
        dT = icp.point_to_point_solve(_sums(step[w, :3], ref_c[ids[w], :3]))
        T_iter = _mul4(dT, T_iter)
        trace.append((np.float32(limit), int(w.sum())))
        it += 1
        counter += 1
        if counter >= cfg.max_iterations:         # CounterTransformationChecker
            break
        rot7.append(abs(_rotation_distance(T_iter, hist[-1])))
        hist.append(T_iter.copy())
        n = len(hist)
        if n > smooth:                            # DifferentialTransformationChecker (float, hostmath::checker_check)
            rot, trans = np.float32(0), np.float32(0)
            for i in range(n - 1, n - smooth - 1, -1):
                rot = np.float32(rot + rot7[i])
                dx, dy, dz = (hist[i][:3, 3] - hist[i - 1][:3, 3]).astype(np.float32)
                trans = np.float32(trans + abs(np.sqrt(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))))
            rot = np.float32(rot / np.float32(smooth))
            trans = np.float32(trans / np.float32(smooth))
            if rot < np.float32(cfg.min_diff_rot) and trans < np.float32(cfg.min_diff_trans):
                converged = True
                break
    Tmean = np.eye(4, dtype=np.float32)
    Tmean[:3, 3] = mean
    return _mul4(Tmean, _mul4(T_iter, T_rm_in)), it, converged, trace


def _yaml_cfg():
    c = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(c))
    return c


@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


def _p2p_handle(icp_mod):
    return icp_mod.IcpHandle(None, 0, "PointToPointErrorMinimizer")


def test_host_loop_recovers_the_synthetic_motion(oracle, pair64k):
    """The test-side loop on its own (no GPU): where the point-to-point chain ends on pair64k, which sets the
    plausibility bound of the device test below."""
    from laser_slam_amd import icp
    rf, _ = oracle.sampling_surface_normal(pair64k["ref"], 10, 0.5, 4)
    keep = oracle.random_sampling(len(pair64k["rd"]), 0.5, -1)
    T, it, conv, _ = host_p2p_icp(oracle, pair64k["rd"][keep], rf, pair64k["T_init"], _yaml_cfg())
    e0 = synth.pose_error(pair64k["T_init"], pair64k["T_true"])
    e1 = synth.pose_error(T.astype(np.float64), pair64k["T_true"])
    assert icp.check_rigid(T) and 1 < it < 40
    # measured: 10 iterations, stopped by the differential checker, 0.0234 m / 0.0084 rad from the truth (the guess:
    # 0.285 m / 0.026 rad); point-to-point converges slower than point-to-plane, the yaml checker (1e-3 rad / 1e-2 m
    # smoothed over 4 iterations) stops it early.  Bounds: 1.5 x what was measured.
    assert e1[0] < e0[0] and e1[1] < e0[1] and e1[0] < 0.035 and e1[1] < 0.0125, (e0, e1, it, conv)


# ------------------------------------------------------------------------------------------------ GPU

def _compare_with_host_loop(icp_mod, oracle, pair, seed, tol_t, tol_r, ssn=True):
    ref, rd, T_init = pair["ref"], pair["rd"], pair["T_init"]
    cfg = _yaml_cfg()
    if ssn:
        rf, _ = oracle.sampling_surface_normal(ref, 10, 0.5, seed)
        keep = oracle.random_sampling(len(rd), 0.5, -1)
    else:
        rf, keep = ref, oracle.random_sampling(len(rd), 0.5, seed)
    Th, ith, convh, trh = host_p2p_icp(oracle, rd[keep], rf, T_init, cfg)
    with _p2p_handle(icp_mod) as h:
        Tg, st = h.compute(rd, ref, T_init, 0.5, 10 if ssn else 0, 0.5, seed=seed)
        trg = [(np.float32(t["limit"]), int(t["n_used"])) for t in h.trace()]
    assert (st.iterations, st.converged) == (ith, int(convh)), (st.iterations, st.converged, ith, convh)
    assert trg == trh
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    assert dt <= tol_t and dr <= tol_r, (dt, dr)
    return Tg, st


@pytest.mark.gpu
def test_device_loop_matches_host_loop_4k(icp_mod, oracle, pair4k):
    _compare_with_host_loop(icp_mod, oracle, pair4k, 4, 1e-5, 1e-6)


@pytest.mark.gpu
def test_device_loop_matches_host_loop_64k_and_is_plausible(icp_mod, oracle, pair64k):
    Tg, st = _compare_with_host_loop(icp_mod, oracle, pair64k, 4, 1e-4, 1e-5)
    e0 = synth.pose_error(pair64k["T_init"], pair64k["T_true"])
    e1 = synth.pose_error(Tg.astype(np.float64), pair64k["T_true"])
    assert e1[0] < e0[0] and e1[1] < e0[1] and e1[0] < 0.035 and e1[1] < 0.0125, (e0, e1)   # (see the host loop's test)


@pytest.mark.gpu
def test_device_loop_matches_host_loop_full_size(icp_mod, oracle):
    """configs[1] size (the 1 M-point pair bench.py uses), the chain without a reference filter."""
    ref, rd, T_true, T_init = synth.scan_pair(16384)
    _compare_with_host_loop(icp_mod, oracle, dict(ref=ref, rd=rd, T_init=T_init), 5, 1e-4, 1e-5, ssn=False)


@pytest.mark.gpu
def test_point_to_point_sums_match_numpy(icp_mod, oracle, pair4k):
    ref, rd = pair4k["ref"], pair4k["rd"]
    with _p2p_handle(icp_mod) as h:
        h.set_reference(ref, None)
        mean = h.reference_mean()
        ref_c = ref.copy()
        ref_c[:, :3] -= mean
        T = synth.colmajor(pair4k["T_init"]).copy()
        T[12:15] -= mean
        ids, d2 = oracle.KdTree(ref_c).nn(oracle.transform_points(T, rd), threads=16)
        rc, limit = oracle.trim_limit(d2, 0.75)
        s = h.point_to_point(rd, T, ids, d2, limit)
    p = oracle.transform_points(T, rd)
    w = d2 <= np.float32(limit)
    want = _sums(p[w, :3], ref_c[ids[w], :3])
    assert s[27] == want[27] == int(w.sum())
    assert (s[15:27] == 0).all()
    # relative to the sum of the terms' magnitudes (the entries of sum q p^T may cancel)
    pd, qd = p[w, :3].astype(np.float64), ref_c[ids[w], :3].astype(np.float64)
    mag = np.concatenate([np.abs(pd).sum(0), np.abs(qd).sum(0), np.einsum("na,nc->ac", np.abs(qd), np.abs(pd)).ravel()])
    assert (np.abs(s[0:15] - want[0:15]) <= 1e-12 * mag).all()
    assert abs(s[28] - want[28]) <= 1e-12 * want[28]


@pytest.mark.gpu
def test_chain_without_reference_filter_is_the_reference_as_given(icp_mod, pair64k):
    ref, rd, T_init = pair64k["ref"], pair64k["rd"], pair64k["T_init"]
    with _p2p_handle(icp_mod) as h:
        h.set_reference(ref, None)
        Ta, sta = h.align(rd, T_init)
        Tc, stc = h.compute(rd, ref, T_init, -1.0, 0, 0.5, seed=3)            # no filter module at all: no draw
        assert h.info().n_reference == len(ref)
        h.cloud_upload(0, ref)
        h.cloud_upload(1, rd)
        Tk, stk = h.compute_clouds(1, [0], None, T_init, -1.0, 0, 0.5, seed=3)
        Tu, stu = h.compute_clouds_upload(2, rd, [0], None, T_init, -1.0, 0, 0.5, seed=3)
    assert sta.iterations == stc.iterations == stk.iterations == stu.iterations > 1
    for T in (Tc, Tk, Tu):
        assert np.array_equal(Ta, T)
    # point-to-plane still needs its normals: ssn_knn 0 is a configuration error there
    with icp_mod.IcpHandle() as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, 0.5, 0, 0.5, seed=3)
        assert e.value.code == _lib.BAD_CONFIG


@pytest.mark.gpu
def test_align_batch_and_split_scan(icp_mod, pair64k):
    pairs = []
    for i, n_az in enumerate([96, 160, 64, 128, 112]):
        ref, rd, _Tt, Ti = synth.scan_pair(n_az, noise_seeds=(3000 + i, 4000 + i), guess_seed=3000 + i)
        pairs.append((ref, None, rd, Ti))
    refs, nrms, rds, Tis = map(list, zip(*pairs))
    results = []
    for pool in (1, 4):
        hs = [_p2p_handle(icp_mod) for _ in range(pool)]
        T, st, rc = icp_mod.align_batch(hs, refs, nrms, rds, Tis)
        for h in hs:
            h.close()
        assert list(rc) == [0] * len(pairs) and all(s.iterations > 1 for s in st)
        results.append(T)
    assert np.array_equal(results[0], results[1])
    # world-1 communicator: the sums are all-reduced and k_icp_update runs as its own launch; the fused select is off in
    # that mode, so the summation order differs -- same limits and counts, T within 1e-6
    with _p2p_handle(icp_mod) as h:
        h.set_reference(pair64k["ref"], None)
        T0, st0 = h.align(pair64k["rd"], pair64k["T_init"])
        tr0 = [(t["limit"], t["n_used"]) for t in h.trace()]
        h.comm_init(0, 1, icp_mod.comm_unique_id())
        T1, st1 = h.align(pair64k["rd"], pair64k["T_init"])
        tr1 = [(t["limit"], t["n_used"]) for t in h.trace()]
    assert st0.iterations == st1.iterations and tr0 == tr1
    assert np.abs(T0 - T1).max() <= 1e-6


@pytest.mark.gpu
def test_icp_facade_runs_a_point_to_point_yaml(icp_mod, pair64k):
    o = icp_mod.ICP()
    o.load_from_yaml(io.StringIO(_without_reference_filter(P2P_YAML)))
    o.chain.seed = 8
    T = o.compute(pair64k["rd"], pair64k["ref"], pair64k["T_init"])
    e0 = synth.pose_error(pair64k["T_init"], pair64k["T_true"])
    e1 = synth.pose_error(T.astype(np.float64), pair64k["T_true"])
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)
    assert o.last_stats.iterations > 1
