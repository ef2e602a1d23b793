"""SurfaceNormalDataPointsFilter as the reference filter: loaders, config layout, the host version against an independent
float64 model and known answers (CPU); the device filter against the host version and ICP.compute end to end (GPU).

The contract is in include/lsgpu_icp.h: everything is taken on the cloud centred on its float mean, neighbours in
ascending d2 with ties to the smaller original index, box_normal's arithmetic, (0, 1, 0) for a degenerate
neighbourhood."""
import ctypes as C
import glob
import io
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REST = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
        "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n"
        "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n"
        "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
        "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
        "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
        "      smoothLength: 4\n")
SSN = "  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n"


def _sn(params=None):
    if params is None:
        return "  - SurfaceNormalDataPointsFilter\n"
    return "  - SurfaceNormalDataPointsFilter:\n" + "".join(f"      {k}: {v}\n" for k, v in params.items())


def _yaml(ref_modules, rest=REST):
    return "referenceDataPointsFilters:\n" + ref_modules + rest


REFUSED = [({"knn": 10, "epsilon": 1}, "epsilon"), ({"knn": 10, "maxDist": 2.0}, "maxDist"),
           ({"knn": 10, "keepDensities": 1}, "keepDensities"), ({"knn": 10, "keepNormals": 0}, "keepNormals"),
           ({"knn": 2}, "knn"), ({"knn": 33}, "knn")]


# ------------------------------------------------------------------------------------------------ CPU: loaders, layout

def test_python_loader_takes_the_module():
    from laser_slam_amd import icp
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 10}))))
    assert o.chain.reference_normal_knn == 10 and o.chain.surface_normal_knn == 0
    o.load_from_yaml(io.StringIO(_yaml(_sn())))
    assert o.chain.reference_normal_knn == 5 and o.chain.surface_normal_knn == 0          # the module's default
    o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 7, "epsilon": 0, "maxDist": "inf", "keepNormals": 1, "keepDensities": 0}))))
    assert o.chain.reference_normal_knn == 7
    for mini in ("PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer"):
        o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 12}), REST.replace("PointToPlaneErrorMinimizer", mini))))
        assert o.chain.reference_normal_knn == 12 and o.chain.error_minimizer == mini
    for params, word in REFUSED:
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(_yaml(_sn(params))))
        assert e.value.code == _lib.BAD_CONFIG, params
        assert "SurfaceNormalDataPointsFilter" in str(e.value) and word in str(e.value), str(e.value)
    for two in (SSN + _sn({"knn": 10}), _sn({"knn": 10}) + SSN, _sn({"knn": 10}) + _sn({"knn": 5})):
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(_yaml(two)))
        assert e.value.code == _lib.BAD_CONFIG
    # neither filter with the point-to-plane minimizer: still refused, for the normals
    with pytest.raises(_lib.LsgpuError) as e:
        o.load_from_yaml(io.StringIO(REST))
    assert "required" in str(e.value)
    assert "SamplingSurfaceNormalDataPointsFilter" in str(e.value) and " SurfaceNormalDataPointsFilter" in str(e.value)
    with pytest.raises(_lib.LsgpuError) as e:                       # not an integer: refused, as the C++ loader does
        o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 5.7}))))
    assert e.value.code == _lib.BAD_CONFIG and "knn" in str(e.value)
    # the sampling filter loads as before
    o.load_from_yaml(io.StringIO(_yaml(SSN)))
    assert o.chain.reference_normal_knn == 0 and o.chain.surface_normal_knn == 10
    assert icp.ChainConfig().reference_normal_knn == 0


# what the golden chains of tests/golden/ loaded to on the parent commit (dataclasses.asdict of ICP.chain)
_GOLDEN_BASE = dict(reading_sampling_prob=0.5, surface_normal_knn=10, surface_normal_ratio=0.5, trim_ratio=0.75,
                    max_iterations=40, min_diff_rot=0.001, min_diff_trans=0.01, smooth_length=4, seed=-1,
                    error_minimizer="PointToPlaneErrorMinimizer", matcher_knn=1, matcher_max_dist=0.0,
                    outlier_max_dist=0.0, outlier_min_dist=0.0, outlier_median_factor=0.0, extra={})
GOLDEN_CHAINS = {
    "icp_chain.yaml": _GOLDEN_BASE,
    "icp_chain_tight.yaml": dict(_GOLDEN_BASE, min_diff_rot=1e-05, min_diff_trans=0.0001),
}


def test_golden_yaml_load_as_before():
    """Every golden ICP chain loads to the ChainConfig it loaded to before, the new field 0 (the other *.yaml files
    there are input filter chains, which ICP.load_from_yaml never took)."""
    import dataclasses
    from laser_slam_amd import icp
    names = {os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.yaml"))}
    assert names == set(GOLDEN_CHAINS) | {"input_filters.yaml", "input_filters_none.yaml"}
    for n, want in GOLDEN_CHAINS.items():
        o = icp.ICP()
        o.load_from_yaml(os.path.join(ROOT, "tests", "golden", n))
        assert dataclasses.asdict(o.chain) == dict(want, reference_normal_knn=0), n


def test_cpp_loader_takes_the_module(tmp_path):
    exe = str(tmp_path / "surface_normal_loader_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", ROOT,
                           os.path.join(ROOT, "tests", "cpp", "surface_normal_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp",
                           "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "surface_normal_loader_check: ok" in r.stdout, r.stdout + r.stderr


def test_chain_config_layout_and_exclusion():
    c = _lib.ChainCfg()
    assert C.sizeof(c) == 24
    assert [(_lib.ChainCfg.reading_prob.offset), _lib.ChainCfg.ssn_knn.offset, _lib.ChainCfg.ssn_ratio.offset,
            _lib.ChainCfg.sn_knn.offset, _lib.ChainCfg.seed.offset] == [0, 4, 8, 12, 16]
    L = _lib.lib()
    for preset in (L.lsgpu_chain_config_yaml, L.lsgpu_chain_config_default):
        preset(C.byref(c))
        assert c.sn_knn == 0 and c.ssn_knn > 0
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_PLANE) == _lib.OK
        c.sn_knn = 10                                                # both reference filters at once
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_PLANE) == _lib.BAD_CONFIG
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_POINT) == _lib.BAD_CONFIG
        c.ssn_knn = 0
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_PLANE) == _lib.OK
        for bad in (-1, 1, 2, 33):
            c.sn_knn = bad
            assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_POINT) == _lib.BAD_CONFIG
        c.sn_knn = 0                                                 # no filter at all: point-to-point only
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_POINT) == _lib.OK
        assert L.lsgpu_chain_config_check(C.byref(c), _lib.MINIMIZER_POINT_TO_PLANE) == _lib.BAD_CONFIG
    assert L.lsgpu_abi_version() == 4
    for s in ("lsgpu_icp_filter_reference_normals", "lsgpu_filter_surface_normal", "lsgpu_chain_config_check"):
        assert s in _lib.ABI_SYMBOLS and hasattr(L, s)


# ------------------------------------------------------------------------------------------------ CPU: the host version

@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    """knn_brute (tests/cpp/knn_brute.c): exact k-NN in the device's arithmetic, 16 threads at most.  Its list length is
    a compile-time constant of 16, this filter needs up to knn + 1 = 33: the same source is compiled with that one
    constant raised."""
    tmp = tmp_path_factory.mktemp("knn_brute")
    so = str(tmp / "libknn_brute.so")
    src = open(os.path.join(ROOT, "tests", "cpp", "knn_brute.c")).read()
    assert src.count("#define KNN_BRUTE_MAX_K 16") == 1
    with open(tmp / "knn_brute.c", "w") as f:
        f.write(src.replace("#define KNN_BRUTE_MAX_K 16", "#define KNN_BRUTE_MAX_K 40"))
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           str(tmp / "knn_brute.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    L.knn_brute.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def knn(ref_xyz1, q_xyz1, k):
        r = np.ascontiguousarray(ref_xyz1, np.float32)
        q = np.ascontiguousarray(q_xyz1, np.float32)
        ids = np.empty((len(q), k), np.int32)
        d2 = np.empty((len(q), k), np.float32)
        assert L.knn_brute(r.ctypes.data, len(r), q.ctypes.data, len(q), k, 16, ids.ctypes.data, d2.ctypes.data) == 0
        return ids, d2
    return knn


def centred(xyz1):
    """The contract's coordinates: float mean from double sums, one float subtraction per coordinate."""
    a = np.ascontiguousarray(xyz1, np.float32)
    mean = (a[:, :3].astype(np.float64).sum(axis=0) / len(a)).astype(np.float32)
    out = a.copy()
    out[:, :3] = a[:, :3] - mean
    return out


@pytest.fixture(scope="module")
def scans():
    return {n: synth.scan_pair(n)[0] for n in (256, 1024)}


def model_normals(c, ids):
    """float64: covariance of each neighbourhood, eigenvector of the smallest eigenvalue (numpy.linalg.eigh)."""
    p = c[:, :3].astype(np.float64)[ids]                      # n x k x 3
    e = p - p.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", e, e)
    w, v = np.linalg.eigh(cov)
    return v[:, :, 0]


def angle(a, b):
    """angle between two fields of unit vectors, up to sign [rad]"""
    a = a.astype(np.float64); b = b.astype(np.float64)
    cr = np.linalg.norm(np.cross(a, b), axis=1)
    dt = np.abs(np.sum(a * b, axis=1))
    return np.arctan2(cr, dt)


@pytest.mark.parametrize("n_az", [256, 1024])
@pytest.mark.parametrize("knn", [5, 10, 20])
def test_host_filter_against_float64_model(scans, brute, n_az, knn):
    """Bound 1e-3 rad: a float32 restatement of the mean / covariance against the float64 model differs by at most
    9.3e-5 rad over these six cases; ten times that for the summation order.  Observed maxima of the host version
    [rad]: knn 5 4.6e-5 (256) / 9.0e-5 (1024), knn 10 3.8e-7 / 9.5e-6, knn 20 4.6e-7 / 3.2e-6; points left out of the
    id comparison for tied distances: 0, 0, 2, 0, 2, 2."""
    from scipy.spatial import cKDTree
    from laser_slam_amd import icp
    ref = scans[n_az]
    n = len(ref)
    nrm, ids, d2 = icp.surface_normal(ref, knn, with_neighbours=True)
    c = centred(ref)
    bids, bd2 = brute(c, c, knn + 1)
    # distance lists: bit-equal to the brute force on the contract's coordinates, nothing left out
    assert np.array_equal(d2.view(np.uint32), bd2[:, :knn].view(np.uint32))
    assert np.array_equal(ids[:, 0], np.arange(n))                               # self first, at distance 0
    assert np.all(d2[:, 0] == 0.0)
    # ids: for every point whose knn + 1 smallest distances are pairwise distinct; the rest at most 0.1 %
    distinct = np.all(np.diff(bd2, axis=1) > 0, axis=1)
    print(f"n {n} knn {knn}: tied points {int((~distinct).sum())}")
    assert (~distinct).sum() <= 1e-3 * n, "vacuous: too many points left out of the id comparison"
    assert np.array_equal(ids[distinct], bids[distinct, :knn])
    # ... and against an independent float64 search
    _, kid = cKDTree(c[:, :3].astype(np.float64)).query(c[:, :3].astype(np.float64), k=knn)
    assert np.array_equal(np.sort(ids[distinct], axis=1), np.sort(kid[distinct], axis=1))
    # normals against the float64 model, nothing left out (the model on the filter's own neighbourhoods: where distances
    # tie, the contract's rule picks the members)
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    worst = float(angle(nrm, model_normals(c, ids)).max())
    print(f"n {n} knn {knn}: max angle to the float64 model {worst:.3e} rad")
    assert worst <= 1e-3


def test_host_filter_known_answers(brute):
    from laser_slam_amd import icp
    rng = np.random.default_rng(5)
    # a lattice in the plane through (1, 2, 3) spanned by u, v, jittered in the plane: +- the plane's normal
    u = np.array([1.0, 2.0, 0.5]); u /= np.linalg.norm(u)
    w = np.array([0.3, -0.2, 1.0]); w -= u * (u @ w); w /= np.linalg.norm(w)
    nn = np.cross(u, w)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40)), -1).reshape(-1, 2) * 0.1 + rng.uniform(-0.03, 0.03, (1600, 2))
    plane = np.ones((1600, 4), np.float32)
    plane[:, :3] = np.array([1.0, 2.0, 3.0]) + g[:, :1] * u + g[:, 1:] * w
    for knn in (5, 10, 20):
        nrm = icp.surface_normal(plane, knn)
        assert angle(nrm, np.broadcast_to(nn, nrm.shape)).max() <= 1e-3
    # all points on one line: every neighbourhood fails the rank test -> the stated value, every point kept
    line = np.ones((200, 4), np.float32)
    line[:, :3] = np.arange(200)[:, None] * np.array([0.25, 0.5, -0.125], np.float32)     # exact in float
    nrm = icp.surface_normal(line, 5)
    assert nrm.shape == (200, 3) and np.array_equal(nrm, np.broadcast_to(np.float32([0, 1, 0]), (200, 3)))
    # every point twice: ties everywhere; deterministic, and the distance lists still those of the brute force
    base = synth.scan_pair(64)[0][:1500]
    dup = np.concatenate([base, base])
    a = icp.surface_normal(dup, 10, with_neighbours=True)
    b = icp.surface_normal(dup, 10, with_neighbours=True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    c = centred(dup)
    assert np.array_equal(a[2].view(np.uint32), brute(c, c, 10)[1].view(np.uint32))
    assert np.array_equal(a[1][:, 0], np.concatenate([np.arange(1500), np.arange(1500)]))  # ties: the smaller index
    # n = knn works, n = knn - 1 is a bad argument
    small = plane[:7]
    nrm, ids, d2 = icp.surface_normal(small, 7, with_neighbours=True)
    assert np.array_equal(np.sort(ids, axis=1), np.broadcast_to(np.arange(7), (7, 7)))
    with pytest.raises(_lib.LsgpuError) as e:
        icp.surface_normal(plane[:6], 7)
    assert e.value.code == _lib.BAD_ARG
    for knn in (2, 33, 0, -4):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.surface_normal(plane, knn)
        assert e.value.code == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ GPU

def _same(dev, host):
    for x, y, what in zip(dev, host, ("normals", "ids", "d2")):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), what


@pytest.mark.gpu
@pytest.mark.parametrize("knn", [3, 5, 10, 16, 32])
def test_device_filter_equals_host_filter(scans, knn):
    from laser_slam_amd import icp
    with icp.IcpHandle(device=0) as h:
        for n_az in (256, 1024):
            ref = scans[n_az]
            _same(h.filter_reference_normals(ref, knn, with_neighbours=True), icp.surface_normal(ref, knn, with_neighbours=True))
            # without ids: the same normals
            assert np.array_equal(h.filter_reference_normals(ref, knn).view(np.uint32),
                                  icp.surface_normal(ref, knn).view(np.uint32))
        # the known answers on the device: a line (degenerate), duplicates (ties), n = knn, n = knn - 1
        line = np.ones((200, 4), np.float32)
        line[:, :3] = np.arange(200)[:, None] * np.array([0.25, 0.5, -0.125], np.float32)
        _same(h.filter_reference_normals(line, knn, with_neighbours=True), icp.surface_normal(line, knn, with_neighbours=True))
        base = scans[256][:3000]
        dup = np.concatenate([base, base])
        _same(h.filter_reference_normals(dup, knn, with_neighbours=True), icp.surface_normal(dup, knn, with_neighbours=True))
        few = scans[256][:knn]
        _same(h.filter_reference_normals(few, knn, with_neighbours=True), icp.surface_normal(few, knn, with_neighbours=True))
        with pytest.raises(_lib.LsgpuError) as e:
            h.filter_reference_normals(scans[256][:knn - 1], knn)
        assert e.value.code == _lib.BAD_ARG
        for bad in (2, 33, -4):
            with pytest.raises(_lib.LsgpuError) as e:
                h.filter_reference_normals(scans[256], bad, with_neighbours=True)
            assert e.value.code == _lib.BAD_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("knn", [3, 5, 10, 16, 32])
def test_device_filter_on_a_three_scan_submap(knn):
    """compute_clouds' reference: three scans moved into one frame and concatenated (overlapping surfaces, far-field
    points of one scan between the rings of another)."""
    from laser_slam_amd import icp
    scene = synth.scan_pair(256)
    a, b = scene[0], scene[1]
    with icp.IcpHandle(device=0) as h:
        T1 = synth.se3(0.4, 0.1, 0.0, yaw=0.02).astype(np.float32)
        T2 = synth.se3(-0.3, 0.2, 0.05, yaw=-0.03).astype(np.float32)
        sub = np.concatenate([a, h.transform_points(T1, b), h.transform_points(T2, a)])
        _same(h.filter_reference_normals(sub, knn, with_neighbours=True), icp.surface_normal(sub, knn, with_neighbours=True))


def _oracle_run(ref, rd, T_init, knn, seed, prob=0.5):
    """The oracle's own loop on the unfiltered reference with the host filter's normals and the reading sampled by the
    oracle's RandomSampling with the same seed (the reference filter draws nothing)."""
    from laser_slam_amd import icp
    from oracle import oracle_py as O
    nrm = icp.surface_normal(ref, knn)
    keep = O.random_sampling(len(rd), prob, seed)
    return O.icp_compute(O.config_yaml(accum_double=1), rd[keep], ref, nrm, synth.colmajor(T_init), 64)


@pytest.mark.gpu
@pytest.mark.parametrize("n_az", [256, 1024])
def test_compute_with_the_filter_equals_the_oracle_loop(n_az):
    from laser_slam_amd import icp
    ref, rd, _T_true, T_init = synth.scan_pair(n_az)
    o = icp.ICP(device=0)
    o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 10}))))
    o.chain.seed = 11
    T = o.compute(rd, ref, T_init)
    st = o.last_stats
    tr = o._handle.trace(64)
    rc, To, sto, tro = _oracle_run(ref, rd, T_init, 10, 11)
    assert rc == 0
    assert st.iterations == sto.iterations
    for i, (a, b) in enumerate(zip(tr, tro)):
        assert np.float32(a["limit"]).view(np.uint32) == np.float32(b["limit"]).view(np.uint32), i
        assert a["n_used"] == b["n_used"], i
    dt, dr = synth.pose_error(synth.from_colmajor(To), T.astype(np.float64))
    print(f"n_az {n_az}: {st.iterations} iterations, |dt| {dt:.2e} m, |dr| {dr:.2e} rad")
    assert dt <= 1e-4 and dr <= 1e-5
    # the handle-level call with the chain field, clouds resident: the same result; both filters at once: refused
    h = o._handle
    T2, _ = h.compute(rd, ref, T_init, 0.5, 0, 0.5, 11, sn_knn=10)
    assert np.array_equal(T2.view(np.uint32), T.view(np.uint32))
    h.cloud_upload(0, rd); h.cloud_upload(1, ref)
    T3, _ = h.compute_clouds(0, [1], None, T_init, 0.5, 0, 0.5, 11, sn_knn=10)
    assert np.array_equal(T3.view(np.uint32), T.view(np.uint32))
    T4, _ = h.compute_clouds_upload(2, rd, [1], None, T_init, 0.5, 0, 0.5, 11, sn_knn=10)
    assert np.array_equal(T4.view(np.uint32), T.view(np.uint32))
    with pytest.raises(_lib.LsgpuError) as e:
        h.compute(rd, ref, T_init, 0.5, 10, 0.5, 11, sn_knn=10)
    assert e.value.code == _lib.BAD_CONFIG
    with pytest.raises(_lib.LsgpuError) as e:
        h.compute(rd, ref[:9], T_init, 0.5, 0, 0.5, 11, sn_knn=10)
    assert e.value.code == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ chains that only consume the normals
# The test-side loop of tests/test_knn_matcher.py / tests/test_outlier_chain.py, re-stated for the point-to-plane
# minimizer: exact neighbours, KDTreeMatcher maxDist, Trimmed- / MaxDistOutlierFilter, the oracle's minimizer and checkers.

INF = np.float32(np.inf)


def _mul4(a, b):
    """a @ b in float32 with the operation order of hostmath::mul4 / the oracle's mat4_mul (4x4, row-major numpy)."""
    s = a[:, 0:1] * b[0:1, :]
    s = s + a[:, 1:2] * b[1:2, :]
    s = s + a[:, 2:3] * b[2:3, :]
    s = s + a[:, 3:4] * b[3:4, :]
    return s.astype(np.float32)


def _sq(v):
    return np.float32(np.float32(v) * np.float32(v))             # one float multiply


def host_chain_icp(oracle, nn, rd, ref, nrm, T_init, k, chain, mean):
    """ICP::compute steps 2-7 on an already filtered pair, chain = {trim, matcher (KDTreeMatcher maxDist), max
    (MaxDistOutlierFilter)}: centre the reference on `mean`, move the reading by T_refMean_dataIn, then per iteration
    {transform, exact k-NN, matches beyond the matcher's maxDist invalid, trimmed limit over the valid matches, the
    smaller of the upper limits, point-to-plane on the kept pairs, checkers of icp_default.yaml}.
    -> (T 4x4 float32, iterations, converged, [(limit, n_used)], [share of invalid matches])."""
    from laser_slam_amd import icp
    ratio, smooth, max_it, lim_rot, lim_trans = chain.get("trim", 1.0), 4, 40, 0.001, 0.01
    mean = np.asarray(mean, np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T_rm_in = np.asarray(T_init, np.float32).copy()
    T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
    reading = oracle.transform_points(synth.colmajor(T_rm_in), rd)
    T_iter = np.eye(4, dtype=np.float32)
    hist, rot7 = [T_iter.copy()], [np.float32(0)]
    it, converged, trace, invalid = 0, False, [], []
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = nn(ref_c, step, k)
        ids, d2 = ids.copy(), d2.copy()
        if chain.get("matcher"):
            out = ~(d2 <= _sq(chain["matcher"]))
            ids[out] = -1
            d2[out] = INF
        idf, df = ids.ravel().copy(), d2.ravel().copy()          # Matches, k x N column major, flattened
        invalid.append(1.0 - float(np.isfinite(df).sum()) / df.size)
        rc, limit = oracle.trim_limit(df, ratio)
        assert rc == 0
        limit = np.float32(limit)
        if chain.get("max"):
            limit = min(limit, _sq(chain["max"]))
        pf = np.repeat(step, k, axis=0)                          # the reading point once per match
        rc, _A, _b, _x, dT16, used = oracle.point_to_plane(pf, ref_c, nrm, idf, df, limit, 1)
        assert rc == 0
        T_iter = _mul4(dT16.reshape(4, 4).T, T_iter)
        trace.append((np.float32(limit), int(used)))
        it += 1
        if it >= max_it:                              # CounterTransformationChecker
            break
        rot7.append(abs(np.float32(icp.rotation_distance(T_iter, hist[-1]))))
        hist.append(T_iter.copy())
        n = len(hist)
        if n > smooth:                                # DifferentialTransformationChecker (float, hostmath::checker_check)
            rot, trans = np.float32(0), np.float32(0)
            for i in range(n - 1, n - smooth - 1, -1):
                rot = np.float32(rot + rot7[i])
                dx, dy, dz = (hist[i][:3, 3] - hist[i - 1][:3, 3]).astype(np.float32)
                trans = np.float32(trans + abs(np.sqrt(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))))
            rot = np.float32(rot / np.float32(smooth))
            trans = np.float32(trans / np.float32(smooth))
            if rot < np.float32(lim_rot) and trans < np.float32(lim_trans):
                converged = True
                break
    Tmean = np.eye(4, dtype=np.float32)
    Tmean[:3, 3] = mean
    return _mul4(Tmean, _mul4(T_iter, T_rm_in)), it, converged, trace, invalid


def test_restated_loop_with_one_match_is_the_oracle_loop(brute):
    """The loop above, on this filter's output, against lso_icp_compute: same iterations, limits, counts and T."""
    from laser_slam_amd import icp
    from oracle import oracle_py as O
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    nrm = icp.surface_normal(ref, 10)
    rc, To, sto, tro = O.icp_compute(O.config_yaml(accum_double=1), rd, ref, nrm, synth.colmajor(T_init), 64)
    assert rc == 0
    mean = np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] / len(ref)
    T, it, conv, tr, _inv = host_chain_icp(O, brute, rd, ref, nrm, T_init, 1, dict(trim=0.75), mean)
    assert (it, int(conv)) == (sto.iterations, sto.converged)
    assert tr == [(np.float32(t["limit"]), int(t["n_used"])) for t in tro]
    assert np.array_equal(T, synth.from_colmajor(To).astype(np.float32))


KNN3_REST = REST.replace("    knn: 1\n", "    knn: 3\n")
MAXDIST = dict(trim=0.75, matcher=0.5, max=0.3)
MAXDIST_REST = (REST.replace("    knn: 1\n", "    knn: 1\n    maxDist: 0.5\n")
                .replace("      ratio: 0.75\n", "      ratio: 0.75\n  - MaxDistOutlierFilter:\n      maxDist: 0.3\n"))
CHAIN_CASES = {"knn3": (KNN3_REST, 3, dict(trim=0.75)), "maxdist": (MAXDIST_REST, 1, MAXDIST)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CHAIN_CASES))
@pytest.mark.parametrize("n_az", [256, 1024])
def test_compute_with_the_filter_under_knn3_and_maxdist_chains(brute, case, n_az):
    """`KDTreeMatcher knn: 3`, and KDTreeMatcher maxDist + MaxDistOutlierFilter, on top of this filter: these chains read
    the normals through the k-match / chain instantiations of the normal equations.  Against the re-stated loop on the
    unfiltered reference with the host filter's normals and the reading sampled by lso_random_sampling, same seed."""
    from laser_slam_amd import icp
    from oracle import oracle_py as O
    rest, k, chain = CHAIN_CASES[case]
    assert "knn: 3" in KNN3_REST and "maxDist: 0.5" in MAXDIST_REST and "MaxDistOutlierFilter" in MAXDIST_REST
    ref, rd, _T_true, T_init = synth.scan_pair(n_az)
    o = icp.ICP(device=0)
    o.load_from_yaml(io.StringIO(_yaml(_sn({"knn": 10}), rest)))
    assert o.chain.reference_normal_knn == 10 and o.chain.matcher_knn == k
    assert o.chain.matcher_max_dist == chain.get("matcher", 0.0) and o.chain.outlier_max_dist == chain.get("max", 0.0)
    o.chain.seed = 11
    T = o.compute(rd, ref, T_init)
    st = o.last_stats
    trg = [(np.float32(t["limit"]), int(t["n_used"])) for t in o._handle.trace(64)]
    mean = o._handle.reference_mean()
    keep = O.random_sampling(len(rd), 0.5, 11)
    Th, ith, convh, trh, invalid = host_chain_icp(O, brute, rd[keep], ref, icp.surface_normal(ref, 10), T_init, k, chain, mean)
    print("device", st.iterations, st.converged, trg)
    print("host  ", ith, int(convh), trh, "invalid", invalid[0], invalid[-1])
    if chain.get("matcher"):                                     # not vacuous: the matcher's bound cuts matches
        assert invalid[0] >= 0.01, invalid[0]
    assert (st.iterations, st.converged) == (ith, int(convh))
    assert trg == trh                                            # limit and n_used of every iteration, bit for bit
    dt, dr = synth.pose_error(T.astype(np.float64), Th.astype(np.float64))
    print(f"{case} n_az {n_az}: {st.iterations} iterations, |dt| {dt:.2e} m, |dr| {dr:.2e} rad")
    assert dt <= 1e-4 and dr <= 1e-5


@pytest.mark.gpu
def test_the_filter_consumes_no_draw():
    """The reading filter's draws start where the stream stood: the reading kept behind this reference filter is the
    reading kept by the first draws of the seed."""
    from laser_slam_amd import icp
    ref, rd, _T_true, T_init = synth.scan_pair(128)
    with icp.IcpHandle(device=0) as h:
        h.compute(rd, ref, T_init, 0.5, 0, 0.5, 3, sn_knn=5)
        after = h.filter_reading(rd, 0.5, -1)                      # continues the stream
        keep0 = icp.random_sampling(len(rd), 0.5, 3)
        keep1 = icp.random_sampling(len(rd), 0.5, -1)
        assert np.array_equal(after, rd[keep1]) and len(keep0)
