"""PointToPlaneWithCovErrorMinimizer: the chain loader's row, the host twin of the 6x6 solve, the covariance kernel and the
pass after the loop (include/lsgpu_icp.h "PointToPlaneWithCovErrorMinimizer").

The float64 model is a numpy restatement of the arithmetic the header states; it takes the float32 inputs the library takes.
Geometry: a closed room of 8 x 6 x 3 m seen from inside -- points on its six faces with analytic inward normals, the whole room
turned by yaw 0.3, pitch 0.2, roll 0.1 rad so that no normal component is zero.  cond(H) of that room is about 9; every test
asserts cond(H) <= 20 on the numpy side before it compares anything."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, icp, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

CHAIN = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter: {prob: 0.5}\n"
         "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter: {knn: 10}\n"
         "matcher:\n  KDTreeMatcher: {knn: 1, epsilon: 0}\n"
         "outlierFilters:\n  - TrimmedDistOutlierFilter: {ratio: 0.75}\n"
         "errorMinimizer:\n  %s\n"
         "transformationCheckers:\n  - CounterTransformationChecker: {maxIterationCount: %d}\n"
         "  - DifferentialTransformationChecker: {minDiffRotErr: 0.001, minDiffTransErr: 0.01, smoothLength: 4}\n")
PLAIN, WITH_COV = "PointToPlaneErrorMinimizer", "PointToPlaneWithCovErrorMinimizer"


# ---------------------------------------------------------------------------------------------- geometry and model

def room(n, seed):
    """n points on the faces of the 8 x 6 x 3 m room (face i % 6, uniform on it), inward unit normals; both turned by
    yaw 0.3, pitch 0.2, roll 0.1.  -> (xyz1 (n, 4) float32, normals (n, 3) float32)"""
    rng = np.random.default_rng(seed)
    half = np.array([4.0, 3.0, 1.5])
    p = (rng.random((n, 3)) * 2.0 - 1.0) * half
    nrm = np.zeros((n, 3))
    face = np.arange(n) % 6
    for f in range(6):
        ax, sign = f // 2, 1.0 if f % 2 == 0 else -1.0
        sel = face == f
        p[sel, ax] = sign * half[ax]
        nrm[sel, ax] = -sign
    R = synth.se3(yaw=0.3, pitch=0.2, roll=0.1)[:3, :3]
    xyz1 = np.ones((n, 4), np.float32)
    xyz1[:, :3] = (p @ R.T).astype(np.float32)
    return xyz1, np.ascontiguousarray((nrm @ R.T).astype(np.float32))


def reading_of(n, seed):
    """A reading of the room: its own n points plus 1 cm of noise and a 2 cm offset."""
    xyz1, _ = room(n, seed)
    rng = np.random.default_rng(seed + 1000)
    out = xyz1.copy()
    out[:, :3] += (rng.normal(0.0, 0.01, (n, 3)) + np.array([0.02, 0.0, 0.0])).astype(np.float32)
    return out


def centre(ref):
    """The reference on its mean as lsgpu_icp_set_reference centres it -> (centred (n, 3) float32, mean float32)"""
    mean = (ref[:, :3].astype(np.float64).sum(0) / len(ref)).astype(np.float32)
    return ref[:, :3] - mean, mean


def step_params(dT):
    """{alpha, beta, gamma, t} of the 4x4 step, the angles in double and rounded to float32 (what the kernel is handed)"""
    dT = np.asarray(dT, np.float32).astype(np.float64)
    beta = -np.arcsin(dT[2, 0])
    alpha = np.arctan2(dT[2, 1], dT[2, 2])
    gamma = np.arctan2(dT[1, 0] / np.cos(beta), dT[0, 0] / np.cos(beta))
    w = np.array([alpha, beta, gamma]).astype(np.float32).astype(np.float64)
    return w, dT[:3, 3].copy()


def model_sums(p, q, n, keep, dT):
    """The 44 sums in float64.  p: the reading points at the pose (k, 3), q / n: their matches and the matches' normals,
    keep: the pairs that count."""
    w, t = step_params(dT)
    p, q, n = (np.asarray(a, np.float64)[keep] for a in (p, q, n))
    rp = np.linalg.norm(p, axis=1, keepdims=True)
    rq = np.linalg.norm(q, axis=1, keepdims=True)
    u, v = p / rp, q / rq
    m = np.cross(u, n)
    E = (n * (p + np.cross(w, p) + t - q)).sum(1, keepdims=True)
    Nrd = (n * (u + np.cross(w, u))).sum(1, keepdims=True)
    Nrf = -(n * v).sum(1, keepdims=True)
    h = np.hstack([n, rp * m])
    a = np.hstack([n * Nrd, m * (E + rp * Nrd)])
    b = np.hstack([n * Nrf, rq * m * Nrf])
    H, M = h.T @ h, a.T @ a + b.T @ b
    iu = np.triu_indices(6)
    res = (n * (p - q)).sum(1)
    return np.concatenate([H[iu], M[iu], [float(len(p)), float((res * res).sum())]])


def unpack(sums):
    H, M = np.zeros((6, 6)), np.zeros((6, 6))
    iu = np.triu_indices(6)
    H[iu], M[iu] = sums[:21], sums[21:42]
    return H + np.triu(H, 1).T, M + np.triu(M, 1).T


def model_cov(sums, sigma):
    H, M = unpack(sums)
    assert np.linalg.cond(H) <= 20.0, np.linalg.cond(H)
    Hi = np.linalg.inv(H)
    sigma = float(np.float32(sigma))                    # sensor_std_dev is a float of the ABI
    return sigma * sigma * Hi @ M @ Hi


def rel_fro(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


DT = synth.se3(0.004, -0.003, 0.002, yaw=0.002, pitch=-0.001, roll=0.0015).astype(np.float32)


def room_sums(n):
    """The model's sums of a room of n points matched with itself point by point under a small pose and the step DT"""
    ref, nrm = room(n, 11)
    q, _ = centre(ref)
    rd = reading_of(n, 11)
    p = rd[:, :3].astype(np.float64) - centre(ref)[1]
    return model_sums(p, q, nrm, np.ones(n, bool), DT)


# ---------------------------------------------------------------------------------------------- CPU: the loader

def test_loader_takes_the_module_and_fills_the_two_slots():
    import yaml
    base = icp.chain_load(yaml.load(CHAIN % (PLAIN, 40), Loader=yaml.BaseLoader))
    assert base[0] == _lib.OK and list(base[2].reserved) == [0] * 6
    for text, want in ((WITH_COV, 0.01), (WITH_COV + ":\n    sensorStdDev: 0.05", 0.05)):
        rc, why, lc = icp.chain_load(yaml.load(CHAIN % (text, 40), Loader=yaml.BaseLoader))
        assert rc == _lib.OK and why == "", why
        assert lc.reserved[0] == 1 and list(lc.reserved[2:]) == [0] * 4
        assert np.array([lc.reserved[1]], np.int32).view(np.float32)[0] == np.float32(want)
        assert lc.icp.error_minimizer == _lib.MINIMIZER_POINT_TO_PLANE
        sd = C.c_float(-1.0)
        assert _lib.lib().lsgpu_loaded_chain_covariance(C.byref(lc), C.byref(sd)) == 1 and sd.value == np.float32(want)
        other = _lib.LoadedChain.from_buffer_copy(lc)
        for i in range(6):
            other.reserved[i] = 0
        assert bytes(other) == bytes(base[2])           # apart from `reserved`, the document with PointToPlaneErrorMinimizer
        o = icp.ICP()
        o.load_from_yaml(io.StringIO(CHAIN % (text, 40)))
        assert o.chain.covariance == want and o.chain.error_minimizer == PLAIN
    sd = C.c_float(-1.0)
    assert _lib.lib().lsgpu_loaded_chain_covariance(C.byref(base[2]), C.byref(sd)) == 0 and sd.value == -1.0
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(CHAIN % (PLAIN, 40)))
    assert o.chain.covariance is None
    assert C.sizeof(_lib.LoadedChain) == 200 and C.sizeof(_lib.CovarianceCfg) == 16 and C.sizeof(_lib.IcpQuality) == 320
    cc = _lib.CovarianceCfg()
    _lib.lib().lsgpu_covariance_config_default(C.byref(cc))
    assert cc.sensor_std_dev == np.float32(0.01) and list(cc.reserved) == [0, 0, 0]


BAD = [
    (CHAIN % (WITH_COV + ":\n    sensorStdDev: 0.05\n    force2D: 1", 40), WITH_COV),            # an unknown parameter
    (CHAIN % (WITH_COV + ":\n    sensorStdDev: -1", 40), WITH_COV),
    (CHAIN % (WITH_COV + ":\n    sensorStdDev: .inf", 40), WITH_COV),
    (CHAIN % (WITH_COV + ":\n    sensorStdDev: abc", 40), WITH_COV),
    (CHAIN % (WITH_COV + ":\n  " + PLAIN + ":", 40), PLAIN),                                     # a second minimizer
    (CHAIN % (PLAIN + ":\n  " + WITH_COV + ":", 40), WITH_COV),
    ((CHAIN % (WITH_COV, 40)).replace("  - TrimmedDistOutlierFilter: {ratio: 0.75}\n",
                                      "  - TrimmedDistOutlierFilter: {ratio: 0.75}\n  - RobustOutlierFilter: {robustFct: huber}\n"), WITH_COV),
    ((CHAIN % (WITH_COV, 40)).replace("  - TrimmedDistOutlierFilter: {ratio: 0.75}\n",
                                      "  - SurfaceNormalOutlierFilter: {maxAngle: 1.0}\n")
     .replace("  - RandomSamplingDataPointsFilter: {prob: 0.5}\n",
              "  - RandomSamplingDataPointsFilter: {prob: 0.5}\n  - SurfaceNormalDataPointsFilter: {knn: 8}\n"), WITH_COV),
    ((CHAIN % (WITH_COV, 40)).replace("{knn: 1, epsilon: 0}", "{knn: 2, epsilon: 0}"), WITH_COV),
]


def test_loader_refuses_by_name_through_both_python_entries():
    import yaml
    for text, module in BAD:
        rc, why, _ = icp.chain_load(yaml.load(text, Loader=yaml.BaseLoader))
        assert rc == _lib.BAD_CONFIG and module in why, (text, why)
        with pytest.raises(_lib.LsgpuError) as e:
            icp.ICP().load_from_yaml(io.StringIO(text))
        assert e.value.code == _lib.BAD_CONFIG and why in str(e.value)
    # the combinations are refused with the other module named as well
    for i, other in ((6, "RobustOutlierFilter"), (7, "SurfaceNormalOutlierFilter"), (8, "KDTreeMatcher knn")):
        assert other in icp.chain_load(yaml.load(BAD[i][0], Loader=yaml.BaseLoader))[1]
    # ... and the same chains load with PointToPlaneErrorMinimizer: the refusal is the module's
    for i in (6, 7, 8):
        assert icp.chain_load(yaml.load(BAD[i][0].replace(WITH_COV, PLAIN), Loader=yaml.BaseLoader))[0] == _lib.OK


def test_cpp_facade_loads_and_refuses_the_same(tmp_path):
    exe = str(tmp_path / "cov_loader_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "cpp", "cov_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp",
                           "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    docs = str(tmp_path / "bad.docs")
    with open(docs, "wb") as f:
        for text, module in BAD:
            b = text.encode()
            f.write(b"DOC %d %s\n" % (len(b), module.encode()) + b)
    r = subprocess.run([exe, docs], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cov_loader_check: ok %d" % len(BAD) in r.stdout, r.stdout + r.stderr
    # the refusals' texts are the library's, whichever facade asks
    import yaml
    whys = [line[4:] for line in r.stdout.splitlines() if line.startswith("ERR ")]
    assert whys == [icp.chain_load(yaml.load(text, Loader=yaml.BaseLoader))[1] for text, _ in BAD]


# ---------------------------------------------------------------------------------------------- CPU: the host twin

@pytest.mark.parametrize("n", [66, 258, 4098])
def test_host_twin_against_numpy(n):
    sums = room_sums(n)
    want = model_cov(sums, 0.01)
    got = icp.point_to_plane_cov_solve(sums, 0.01)
    err = rel_fro(got, want)
    print("n", n, "cond(H)", np.linalg.cond(unpack(sums)[0]), "relative Frobenius error", err)
    assert err <= 1e-10
    assert np.array_equal(got, got.T)
    assert np.all(np.linalg.eigvalsh(got) > 0)
    half, one = icp.point_to_plane_cov_solve(sums, 0.5), icp.point_to_plane_cov_solve(sums, 1.0)
    assert np.array_equal(4.0 * half, one)


def test_host_twin_refuses_what_is_singular():
    L = _lib.lib()
    sums = room_sums(258)

    def solve(s, sigma=0.01):
        s = np.ascontiguousarray(s, np.float64)
        cov = np.full(36, 7.0)
        rc = L.lsgpu_point_to_plane_cov_solve(s.ctypes.data_as(C.POINTER(C.c_double)), sigma,
                                              cov.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, cov

    assert solve(sums)[0] == _lib.OK
    zero = sums.copy()
    zero[42] = 0.0
    rc, cov = solve(zero)
    assert rc == _lib.NO_CONVERGENCE and np.all(cov == 7.0)
    # one plane with n = (0, 0, 1): H[0][0] = 0 exactly
    rng = np.random.default_rng(5)
    q = np.column_stack([rng.random((200, 2)) * 4.0 - 2.0, np.full(200, 1.5)])
    nrm = np.tile([0.0, 0.0, 1.0], (200, 1))
    plane = model_sums(q + rng.normal(0, 0.01, q.shape), q, nrm, np.ones(200, bool), DT)
    assert plane[0] == 0.0
    rc, cov = solve(plane)
    assert rc == _lib.NO_CONVERGENCE and np.all(cov == 7.0)
    for slot in (0, 20, 21, 41):
        nan = sums.copy()
        nan[slot] = np.nan
        rc, cov = solve(nan)
        assert rc == _lib.NO_CONVERGENCE and np.all(cov == 7.0), slot
    inf = sums.copy()
    inf[30] = np.inf
    assert solve(inf)[0] == _lib.NO_CONVERGENCE
    for sigma in (-1.0, float("nan"), float("inf")):
        assert solve(sums, sigma)[0] == _lib.BAD_CONFIG
    with pytest.raises(_lib.ConvergenceError):
        icp.point_to_plane_cov_solve(zero, 0.01)


# ---------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def clouds():
    ref, nrm = room(4098, 11)
    return dict(ref=ref, nrm=nrm, rd=reading_of(4099, 23), rd_same=reading_of(4098, 11))


@gpu
def test_kernel_against_the_model(clouds):
    ref, nrm, rd = clouds["ref"], clouds["nrm"], clouds["rd"]
    T = synth.se3(0.03, 0.0, 0.0, yaw=np.deg2rad(0.5)).astype(np.float32)
    with icp.IcpHandle() as h:
        h.set_reference(ref, nrm)
        q_all = ref[:, :3] - h.reference_mean()
        assert np.array_equal(q_all, centre(ref)[0])
        for nq in (1, 63, 64, 65, 257, 4099):
            query = rd[:nq].copy()
            query[:, :3] -= h.reference_mean()          # the reference-mean frame
            ids, d2 = h.knn(query, T)
            limit = float(np.sort(d2)[min(nq - 1, int(np.float32(nq) * np.float32(0.7)))])
            ids[6::7] = -1
            keep = (ids >= 0) & (d2 <= np.float32(limit))
            assert nq < 64 or (0 < keep.sum() < (ids >= 0).sum() < nq)      # both skip paths run
            out = h.point_to_plane_cov(query, T, ids, d2, limit, DT)
            again = h.point_to_plane_cov(query, T, ids, d2, limit, DT)
            assert out.tobytes() == again.tobytes()
            p = h.transform_points(T, query)[:, :3]
            safe = np.where(ids >= 0, ids, 0)
            want = model_sums(p, q_all[safe], nrm[safe], keep, DT)
            assert out[42] == want[42] == keep.sum()
            for name, got, mod in (("H", *[unpack(s)[0] for s in (out, want)]), ("M", *[unpack(s)[1] for s in (out, want)])):
                scale = np.sqrt(np.outer(np.diag(mod), np.diag(mod)))
                worst = float(np.max(np.abs(got - mod) / np.where(scale > 0, scale, 1.0))) if keep.any() else 0.0
                print("nq", nq, name, "worst |S_ij - model| / sqrt(S_ii S_jj)", worst)
                assert np.all(np.abs(got - mod) <= 1e-5 * scale), (nq, name)
            assert abs(out[43] - want[43]) <= 1e-5 * want[43]


def _by_hand(h, reading, T_init, trace, sigma):
    """The loop's pass fed by hand from the trace: the last iteration's pre-update pose, lsgpu_knn at that pose, the trace's
    limit, lsgpu_point_to_plane_solve of the trace's sums -> (cov, sums, inputs of the model)"""
    T_rm = np.asarray(T_init, np.float32).copy()
    T_rm[:3, 3] -= h.reference_mean()
    moved = h.transform_points(T_rm, reading)
    T_prev = np.eye(4, dtype=np.float32) if len(trace) == 1 else trace[-2]["T_iter"].reshape(4, 4).T.copy()
    last = trace[-1]
    ids, d2 = h.knn(moved, T_prev)
    dT = icp.point_to_plane_solve(np.concatenate([last["A"][np.triu_indices(6)], last["b"]]))
    sums = h.point_to_plane_cov(moved, T_prev, ids, d2, last["limit"], dT)
    ne = h.normal_eq(moved, T_prev, ids, d2, last["limit"])
    return icp.point_to_plane_cov_solve(sums, sigma), sums, dict(moved=moved, T_prev=T_prev, ids=ids, d2=d2, dT=dT, ne=ne)


@gpu
@pytest.mark.parametrize("max_it", [1, 40])
def test_the_loops_pass(clouds, max_it):
    ref, nrm, rd = clouds["ref"], clouds["nrm"], clouds["rd_same"]
    T_init = np.eye(4, dtype=np.float32)
    plain, cov = icp.ICP(), icp.ICP()
    plain.load_from_yaml(io.StringIO(CHAIN % (PLAIN, max_it)))
    cov.load_from_yaml(io.StringIO(CHAIN % (WITH_COV + ":\n    sensorStdDev: 0.02", max_it)))
    results = []
    for o in (plain, cov):
        h = o.handle
        h.set_reference(ref, nrm)
        T, st = h.align(rd, T_init)
        results.append((T, st, h.trace()))
    (T0, st0, tr0), (T1, st1, tr1) = results
    # the module changes no result
    assert T0.tobytes() == T1.tobytes() and st0.iterations == st1.iterations == len(tr0) == len(tr1)
    assert (st0.converged, st0.final_n_used, st0.final_limit) == (st1.converged, st1.final_n_used, st1.final_limit)
    for a, b in zip(tr0, tr1):
        for key in ("T_iter", "A", "b", "x"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert (a["limit"], a["n_used"], a["stragglers"]) == (b["limit"], b["n_used"], b["stragglers"])
    assert st1.iterations == 1 and st1.converged == 0 if max_it == 1 else st1.iterations > 1 and st1.converged == 1
    h = cov.handle
    q = h.quality()
    assert np.array_equal(cov.covariance, q["covariance"])
    assert q["n_pairs"] == st1.final_n_used == tr1[-1]["n_used"]
    assert q["used_ratio"] == np.float32(q["n_pairs"] / len(rd))
    hand, sums, x = _by_hand(h, rd, T_init, tr1, 0.02)
    assert hand.tobytes() == q["covariance"].tobytes()          # bit for bit the hand-fed kernel-level entries
    assert int(sums[42]) == q["n_pairs"] and sums[43] == q["residual"]
    assert x["ne"][2] == q["n_pairs"]
    print("max_it", max_it, "residual vs lsgpu_normal_eq", abs(q["residual"] - x["ne"][3]) / x["ne"][3])
    assert abs(q["residual"] - x["ne"][3]) <= 1e-10 * x["ne"][3]
    # against the numpy model from the same inputs
    keep = (x["ids"] >= 0) & (x["d2"] <= np.float32(tr1[-1]["limit"]))
    p = h.transform_points(x["T_prev"], x["moved"])[:, :3]
    safe = np.where(x["ids"] >= 0, x["ids"], 0)
    want = model_cov(model_sums(p, centre(ref)[0][safe], nrm[safe], keep, x["dT"]), 0.02)
    err = rel_fro(q["covariance"], want)
    print("max_it", max_it, "iterations", st1.iterations, "relative Frobenius error vs the model", err)
    assert err <= 1e-3
    assert np.array_equal(q["covariance"], q["covariance"].T) and np.all(np.linalg.eigvalsh(q["covariance"]) > 0)
    with pytest.raises(_lib.LsgpuError) as e:                  # a chain without the module has no quality record
        plain.covariance
    assert e.value.code == _lib.BAD_CONFIG


@gpu
def test_compute_clouds_gives_the_quality_of_compute(clouds):
    ref, rd = clouds["ref"], clouds["rd_same"]
    T_init = synth.se3(0.01, 0.0, 0.0).astype(np.float32)
    with icp.IcpHandle(covariance=0.01) as h:
        Ta, sa = h.compute(rd, ref, T_init, seed=3)
        qa = h.quality()
        h.cloud_upload(0, ref)
        h.cloud_upload(1, rd)
        Tb, sb = h.compute_clouds(1, [0], None, T_init, seed=3)
        qb = h.quality()
    assert Ta.tobytes() == Tb.tobytes() and sa.iterations == sb.iterations
    assert qa["covariance"].tobytes() == qb["covariance"].tobytes()
    assert (qa["residual"], qa["n_pairs"], qa["used_ratio"]) == (qb["residual"], qb["n_pairs"], qb["used_ratio"])
    assert qa["n_pairs"] == sa.final_n_used and np.all(np.linalg.eigvalsh(qa["covariance"]) > 0)


@gpu
def test_quality_codes_and_refused_handles(clouds):
    ref, nrm, rd = clouds["ref"], clouds["nrm"], clouds["rd_same"]
    eye = np.eye(4, dtype=np.float32)
    with icp.IcpHandle(outlier_max_dist=1e-6) as h:             # a MaxDistOutlierFilter that keeps nothing
        h.set_reference(ref, nrm)
        with pytest.raises(_lib.LsgpuError) as e:               # not switched on
            h.quality()
        assert e.value.code == _lib.BAD_CONFIG and "lsgpu_icp_set_covariance" in str(e.value)
        h.set_covariance(0.01)
        with pytest.raises(_lib.ConvergenceError):              # no alignment yet
            h.quality()
        with pytest.raises(_lib.ConvergenceError):
            h.align(rd, eye)
        with pytest.raises(_lib.ConvergenceError):              # the last alignment did not converge
            h.quality()
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_covariance(bad)
            assert e.value.code == _lib.BAD_CONFIG and "sensorStdDev" in str(e.value)
        with pytest.raises(_lib.LsgpuError) as e:               # the reverse order of calls
            h.set_robust_filter(icp.RobustConfig())
        assert e.value.code == _lib.BAD_CONFIG and WITH_COV in str(e.value)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_normals(icp.NormalsConfig(max_angle=1.0, reading_normals_given=1))
        assert e.value.code == _lib.BAD_CONFIG and WITH_COV in str(e.value)
    for kwargs, module in ((dict(matcher_knn=3), "KDTreeMatcher knn"), (dict(robust=icp.RobustConfig()), "RobustOutlierFilter"),
                           (dict(error_minimizer="PointToPointErrorMinimizer"), "PointToPointErrorMinimizer")):
        with icp.IcpHandle(**kwargs) as h:
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_covariance(0.01)
            assert e.value.code == _lib.BAD_CONFIG and module in str(e.value) and WITH_COV in str(e.value)


@gpu
def test_switched_off_again_enqueues_what_a_plain_handle_does(clouds):
    ref, nrm, rd = clouds["ref"], clouds["nrm"], clouds["rd_same"]
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.profile_kernels = 1                                     # (knn_launches is counted from the launches' events)
    out = []
    for toggle in (False, True):
        with icp.IcpHandle(cfg) as h:
            if toggle:
                h.set_covariance(0.01)
                h.set_covariance(None)
            h.set_reference(ref, nrm)
            T, st = h.align(rd, np.eye(4, dtype=np.float32))
            out.append((T.tobytes(), st.iterations, st.knn_launches))
            if toggle:
                with pytest.raises(_lib.LsgpuError) as e:
                    h.quality()
                assert e.value.code == _lib.BAD_CONFIG
    assert out[0] == out[1] and out[0][2] > 0
