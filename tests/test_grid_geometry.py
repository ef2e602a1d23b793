"""The voxel-hash pyramid beyond the one geometry every other test builds (bits_per_axis 11, fine_bits 5, h0 0.125 m, the
frame's origin inside the cloud, cell_size 0).

The geometry is chosen on the device by k_ref_stats_final (csrc/lsgpu_grid.hip.h); `predict_geometry` restates its rule
in numpy float32 from the prose of include/lsgpu_icp.h ("The voxel grid's geometry") and DESIGN.md §3.  The CPU tests
assert that every cloud of the case table lands in the branch it is meant for (a change to `synth` must not turn the
cases back into bits 11 unnoticed); every GPU test first asserts that lsgpu_icp_get_info reports exactly the predicted
geometry, then compares the searches, the surface-normal filter, the two minimizers' sums and the whole loop with their
CPU references under the bars of the tests they are taken from (test_gpu_parity, test_knn_matcher, test_outlier_chain,
test_surface_normal_filter, test_point_to_point).

Case table (name: intended bits / fine / h0):
  submap3      three scans 40 m apart in one frame, 290 m                    12 / 4 / 0.125
  scaled4      scan_pair(256) x 4 (exact in float), 868 m                    13 / 3 / 0.125
  scaled8      the same scan x 8, 1736 m                                     13 / 3 / 0.25
  stray        scan_pair(256) plus one return 5 km away                      13 / 3 / 0.5
  cell0.03     cell_size 0.03 on scan_pair(256): 0.03 x 8191 = 245.7 m holds the scan's 217 m, so h0 is NOT doubled
  cell0.02     cell_size 0.02: 0.02 x 8191 = 163.8 m does not, h0 doubles to 0.04    (13 / 3 / 0.04: explicit AND doubled)
  cell0.5      cell_size 0.5                                                 11 / 5 / 0.5
  cell64       cell_size 64: the whole street in a handful of cells          11 / 5 / 64
  cell1e-6     cell_size 1e-6: fifteen doublings                             13 / 3 / 1e-6 x 2^15
  far_origin   scan_pair(256) moved by (2000, -3000, 50) m: origin_inside 0, coordinates on a 2.4e-4 m lattice
  one_point, copies500, line2000   zero and one-dimensional extents (search level only; the line spans 500 m: bits 12)
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

from test_gpu_parity import TOL_R, TOL_T, _check_nn
from test_knn_matcher import _check_knn_k
from test_outlier_chain import _compare as _compare_chain, _device as _device_chain, _kd_nn, host_chain_icp
from test_point_to_point import _sums
from test_surface_normal_filter import _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ------------------------------------------------------------------------------------------------ the restated rule

def predict_geometry(xyz1, cell_size=0.0):
    """What lsgpu_icp_set_reference must choose for this cloud: dict(mean, bits, fine, h0, origin_inside), every step in
    float32 except the coordinate sums, which are double."""
    p = np.ascontiguousarray(xyz1, F)[:, :3]
    mean = (p.astype(np.float64).sum(0) / float(len(p))).astype(F)          # the float mean from the double sums
    lo, hi = p.min(0), p.max(0)                                             # the box as given ...
    mn, mx = (lo - mean).astype(F), (hi - mean).astype(F)                   # ... and in the mean frame
    ext = F(np.max((mx - mn).astype(F)))
    need = F(ext * F(1.0001))
    bits, fine = 11, 5
    h0 = F(cell_size) if cell_size > 0 else F(0.125)
    while bits < 13 and F(h0 * F((1 << bits) - 1)) < need:
        bits, fine = bits + 1, fine - 1
    while F(h0 * F((1 << bits) - 1)) < need:
        h0 = F(h0 * F(2))
    # the frame's own origin against the box as given, widened by a tenth of its extent and a millimetre
    inside = bool((p * p).sum(1).max() > 0)                                 # (a cloud that is only the origin has no direction)
    for d in range(3):
        m = F(F(F(0.1) * F(hi[d] - lo[d])) + F(1e-3))
        if not (F(lo[d] - m) <= 0 <= F(hi[d] + m)):
            inside = False
    return dict(mean=mean, bits=bits, fine=fine, h0=h0, origin_inside=inside, extent=float(ext))


# ------------------------------------------------------------------------------------------------ the case table

FAR = np.array([2000.0, -3000.0, 50.0])
# name -> (bits, fine, h0, origin_inside) the case is meant to reach
INTENDED = {
    "submap3": (12, 4, 0.125, True),
    "scaled4": (13, 3, 0.125, True),
    "scaled8": (13, 3, 0.25, True),
    "stray": (13, 3, 0.5, True),
    "cell0.03": (13, 3, 0.03, True),
    "cell0.02": (13, 3, 0.04, True),
    "cell0.5": (11, 5, 0.5, True),
    "cell64": (11, 5, 64.0, True),
    "cell1e-6": (13, 3, 1e-6 * 2 ** 15, True),
    "far_origin": (11, 5, 0.125, False),
    "one_point": (11, 5, 0.125, False),
    "copies500": (11, 5, 0.125, False),
    "line2000": (12, 4, 0.125, True),
}
LOOP_CASES = [c for c in INTENDED if c not in ("one_point", "copies500", "line2000")]
SEARCH_ONLY = ["one_point", "copies500", "line2000"]
SCALE = {"scaled4": 4.0, "scaled8": 8.0}
CELL = {"cell0.03": 0.03, "cell0.02": 0.02, "cell0.5": 0.5, "cell64": 64.0, "cell1e-6": 1e-6}

_cache = {}


def _reading_of(cloud, T_off, rng):
    """The cloud itself, every second point, moved rigidly, plus 5 mm of noise; and the guess that goes with it."""
    rd = cloud[::2].copy()
    rd[:, :3] = (rd[:, :3].astype(np.float64) @ T_off[:3, :3].T + T_off[:3, 3] + rng.normal(0, 0.005, (rd.shape[0], 3))).astype(F)
    T_init = np.linalg.inv(T_off) @ synth.se3(0.03, 0.02, -0.01, yaw=np.deg2rad(0.4))
    return rd, T_init


def _street():
    """scan_pair(256)'s reference scan, filtered by the host filter (normals), its reading and guess."""
    if "street" not in _cache:
        from laser_slam_amd import icp
        cloud = synth.scan_pair(256)[0]
        rf, rn = icp.sampling_surface_normal(cloud, 10, 1.0, 3)
        rd, T_init = _reading_of(cloud, synth.se3(0.2, 0.1, 0.0, yaw=np.deg2rad(1.5)), np.random.default_rng(31))
        _cache["street"] = (cloud, rf, rn, rd, T_init)
    return _cache["street"]


def case(name):
    """-> dict(ref, nrm, rd, T_init, cell_size, scale): what set_reference / align are handed."""
    if name in _cache:
        return _cache[name]
    from laser_slam_amd import icp
    rng = np.random.default_rng(77)
    c = dict(cell_size=CELL.get(name, 0.0), scale=SCALE.get(name, 1.0))
    if name == "submap3":
        scene = synth.Scene(1234)
        poses = [synth.se3(40.0 * i, 0.3 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(1.0 * i)) for i in range(3)]
        parts = []
        for i, P in enumerate(poses):                        # into the middle scan's frame
            s = synth.hdl64_scan(scene, P, 256, 300 + i)
            Trel = np.linalg.inv(poses[1]) @ P
            s[:, :3] = (s[:, :3].astype(np.float64) @ Trel[:3, :3].T + Trel[:3, 3]).astype(F)
            parts.append(s)
        cloud = np.concatenate(parts)
        c["ref"], c["nrm"] = icp.sampling_surface_normal(cloud, 10, 1.0, 3)
        c["rd"], c["T_init"] = _reading_of(cloud, synth.se3(0.2, 0.1, 0.0, yaw=np.deg2rad(1.5)), rng)
    elif name in SCALE:
        _cloud, rf, rn, rd, T_init = _street()
        s = F(SCALE[name])
        c["ref"], c["rd"] = rf.copy(), rd.copy()
        c["ref"][:, :3] *= s                                 # (a power of two: exact, the scene keeps its structure)
        c["rd"][:, :3] *= s
        c["nrm"] = rn
        c["T_init"] = T_init.astype(F).astype(np.float64)    # the unscaled guess in float, its translation scaled exactly
        c["T_init"][:3, 3] *= float(s)
    elif name == "stray":
        _cloud, rf, rn, rd, T_init = _street()
        c["ref"] = np.concatenate([rf, F([[3000.0, -4000.0, 50.0, 1.0]])])
        c["nrm"] = np.concatenate([rn, F([[0.0, 0.0, 1.0]])])
        c["rd"], c["T_init"] = rd, T_init
    elif name in CELL:
        _cloud, c["ref"], c["nrm"], c["rd"], c["T_init"] = _street()
    elif name == "far_origin":
        cloud, _rf, _rn, rd, T_init = _street()
        far = cloud.copy()
        far[:, :3] = (cloud[:, :3].astype(np.float64) + FAR).astype(F)
        c["ref"], c["nrm"] = icp.sampling_surface_normal(far, 10, 1.0, 3)
        c["rd"] = rd.copy()
        c["rd"][:, :3] = (rd[:, :3].astype(np.float64) + FAR).astype(F)
        S = np.eye(4)
        S[:3, 3] = FAR
        c["T_init"] = S @ T_init @ np.linalg.inv(S)
    elif name == "one_point":
        c["ref"] = F([[3.0, -2.0, 1.0, 1.0]])
    elif name == "copies500":
        c["ref"] = np.tile(F([[3.0, -2.0, 1.0, 1.0]]), (500, 1))
    elif name == "line2000":
        c["ref"] = np.ones((2000, 4), F)
        c["ref"][:, :3] = 0
        c["ref"][:, 0] = 0.25 * np.arange(2000)
    else:
        raise KeyError(name)
    if name in SEARCH_ONLY:
        c["nrm"] = np.tile(F([0.0, 0.0, 1.0]), (len(c["ref"]), 1))          # dummy normals
        q = np.ones((3000, 4), F)
        q[:, :3] = c["ref"][rng.integers(0, len(c["ref"]), 3000), :3] + rng.normal(0, 0.4, (3000, 3))
        c["rd"], c["T_init"] = q, synth.se3(0.05, -0.02, 0.01, yaw=np.deg2rad(0.5))
    c["geom"] = predict_geometry(c["ref"], c["cell_size"])
    _cache[name] = c
    return c


# ------------------------------------------------------------------------------------------------ CPU

def test_restated_rule_on_the_clouds_the_other_tests_build(pair4k, pair64k):
    """The rule itself, on clouds whose outcome is known: every cloud the rest of the suite builds is below
    0.125 x 2047 = 255.875 m and gets 11 / 5 / 0.125; and the rule's edges on boxes made for them."""
    for cloud in (pair4k["ref"], pair64k["ref"], synth.scan_pair(256)[0]):
        g = predict_geometry(cloud)
        assert (g["bits"], g["fine"], g["h0"], g["origin_inside"]) == (11, 5, F(0.125), True) and 150 < g["extent"] < 255.875

    def box(ext, at=(0.0, 0.0, 0.0)):
        b = np.ones((2, 4), F)
        b[0, :3] = at
        b[1, :3] = np.asarray(at) + np.array([ext, 0.0, 0.0])
        return b

    want = [(0.0, (11, 5, 0.125)), (255.0, (11, 5, 0.125)), (255.875, (12, 4, 0.125)),   # (ext x 1.0001 no longer fits)
            (256.0, (12, 4, 0.125)), (511.0, (12, 4, 0.125)), (512.0, (13, 3, 0.125)), (1023.0, (13, 3, 0.125)),
            (1024.0, (13, 3, 0.25)), (2047.0, (13, 3, 0.25)), (2048.0, (13, 3, 0.5)), (5000.0, (13, 3, 1.0))]
    for ext, (bits, fine, h0) in want:
        g = predict_geometry(box(ext))
        assert (g["bits"], g["fine"], g["h0"]) == (bits, fine, F(h0)), (ext, g)
    for cs, ext, (bits, fine, h0) in [(0.5, 1000.0, (11, 5, 0.5)), (0.5, 1024.0, (12, 4, 0.5)), (64.0, 217.0, (11, 5, 64.0)),
                                      (0.03, 217.0, (13, 3, 0.03)), (0.02, 217.0, (13, 3, 0.04)), (-1.0, 217.0, (11, 5, 0.125)),
                                      (1e-6, 217.0, (13, 3, F(F(1e-6) * F(2 ** 15)))), (1e-6, 0.0, (11, 5, F(1e-6)))]:
        g = predict_geometry(box(ext), cs)
        assert (g["bits"], g["fine"], g["h0"]) == (bits, fine, F(h0)), (cs, ext, g)
    # the origin: inside the box, within a tenth of the extent plus a millimetre of it, and beyond
    assert predict_geometry(box(10.0, (-5.0, 0.0, 0.0)))["origin_inside"]
    assert predict_geometry(box(10.0, (0.9, 0.0, 0.0)))["origin_inside"]              # 0.9 <= 0.1 x 10 + 1e-3
    assert not predict_geometry(box(10.0, (1.1, 0.0, 0.0)))["origin_inside"]
    assert not predict_geometry(box(10.0, (-5.0, 0.002, 0.0)))["origin_inside"]       # a flat axis has only its millimetre
    assert predict_geometry(box(10.0, (-5.0, 0.0005, 0.0)))["origin_inside"]
    assert not predict_geometry(box(0.0))["origin_inside"]                            # only the origin itself: no direction
    # the mean is the float of the double sum, not a float sum: 3 x 2^24 + 3 needs more than float's 24 bits on the way
    big = np.ones((4, 4), F)
    big[:, 0] = [16777216.0, 16777216.0, 16777216.0, 3.0]
    assert predict_geometry(big)["mean"][0] == F((3 * 16777216.0 + 3.0) / 4.0)


@pytest.mark.parametrize("name", list(INTENDED))
def test_every_case_lands_in_its_intended_branch(name):
    c = case(name)
    g = c["geom"]
    bits, fine, h0, inside = INTENDED[name]
    h0 = F(F(CELL[name]) * F(2 ** 15)) if name == "cell1e-6" else F(h0)
    assert (g["bits"], g["fine"], g["h0"], g["origin_inside"]) == (bits, fine, h0, inside), (name, g)
    assert (bits, fine, float(h0), inside, c["cell_size"]) != (11, 5, 0.125, True, 0.0)      # never the suite's one geometry
    assert len(c["ref"]) <= 66000                                # the oracle stays quick
    if name == "submap3":
        assert 256.0 < g["extent"] < 511.0, g["extent"]
    if name == "far_origin":                                     # many exact ties after centring: coordinates on a coarse lattice
        assert np.abs(c["ref"][:, :3]).max() > 2048 and len(np.unique(c["ref"][:, 1])) < 0.9 * len(c["ref"])


def test_scaled_cases_are_exact_scalings():
    """Scaling by a power of two commutes with every float operation of the search: the metamorphic check below rests on it."""
    _cloud, rf, _rn, rd, _T = _street()
    for name, s in SCALE.items():
        c = case(name)
        assert np.array_equal(c["ref"][:, :3] / F(s), rf[:, :3]) and np.array_equal(c["rd"][:, :3] / F(s), rd[:, :3])
        assert np.array_equal(c["geom"]["mean"] / F(s), predict_geometry(rf)["mean"])


@pytest.mark.parametrize("name", LOOP_CASES)
def test_the_oracle_converges_on_every_loop_case(oracle, name):
    """What keeps the loop comparison from being vacuous: the oracle's loop runs, and for more than four iterations."""
    c = case(name)
    ocfg = oracle.config_yaml(accum_double=1, min_diff_rot=1e-5, min_diff_trans=1e-4 * c["scale"], num_threads=8)
    rc, _To, sto, _tr = oracle.icp_compute(ocfg, c["rd"], c["ref"], c["nrm"], synth.colmajor(c["T_init"]), 0)
    assert rc == 0 and 4 < sto.iterations <= 40, (name, rc, sto.iterations)


def test_cell_size_refusals():
    """lsgpu_icp_create refuses a NaN or +inf cell_size before the device is touched (so also where there is none);
    <= 0, -inf included, stays "automatic" and any finite positive value is legal -- those reach the device and fail
    here only for want of one."""
    L = _lib.lib()
    c = _lib.IcpConfig()
    for bad in (float("nan"), float("inf")):
        L.lsgpu_icp_config_yaml(C.byref(c))
        c.cell_size = bad
        h = C.c_void_p()
        assert L.lsgpu_icp_create(C.byref(c), 0, C.byref(h)) == _lib.BAD_CONFIG, bad
        assert not h.value
    for good in (0.0, -1.0, float("-inf"), 1e-6, 1e-30, 0.03, 64.0, 1e30):
        L.lsgpu_icp_config_yaml(C.byref(c))
        c.cell_size = good
        h = C.c_void_p()
        rc = L.lsgpu_icp_create(C.byref(c), 0, C.byref(h))
        assert rc in (_lib.OK, _lib.HIP_ERROR), (good, rc)
        if rc == _lib.OK:
            L.lsgpu_icp_destroy(h)
    src = open(os.path.join(ROOT, "include", "lsgpu_icp.h")).read()
    assert "The voxel grid's geometry" in src and "NaN and +inf are LSGPU_BAD_CONFIG" in src   # the rule is stated


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    """knn_brute (tests/cpp/knn_brute.c): exact k-NN in the device's arithmetic, 16 threads at most."""
    so = str(tmp_path_factory.mktemp("knn_brute") / "libknn_brute.so")
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "knn_brute.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    L.knn_brute.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def knn(ref_xyz1, q_xyz1, k):
        r = np.ascontiguousarray(ref_xyz1, F)
        q = np.ascontiguousarray(q_xyz1, F)
        ids = np.empty((len(q), k), np.int32)
        d2 = np.empty((len(q), k), F)
        assert L.knn_brute(r.ctypes.data, len(r), q.ctypes.data, len(q), k, 16, ids.ctypes.data, d2.ctypes.data) == 0
        return ids, d2
    return knn


class _BruteOracle:
    """oracle.brute_nn behind the interface _check_nn asks for (the degenerate clouds go to the brute force, not a tree)."""

    def __init__(self, oracle):
        self._o = oracle

    def KdTree(self, ref_c):
        o = self._o

        class _T:
            def nn(self, q):
                return o.brute_nn(ref_c, q)
        return _T()


def _config(c, tight=True):
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    if tight:
        cfg.min_diff_rot, cfg.min_diff_trans = 1e-5, 1e-4 * c["scale"]
    cfg.cell_size = c["cell_size"]
    return cfg


def _assert_geometry(h, c, name):
    """The case reached its branch on the device: lsgpu_icp_get_info equals the restated rule exactly."""
    info, g = h.info(), c["geom"]
    print(f"{name}: bits {info.bits_per_axis} fine {info.fine_bits} h0 {info.cell_size!r} chunks {info.n_chunks} "
          f"(predicted {g['bits']} {g['fine']} {float(g['h0'])!r}, extent {g['extent']:.1f} m)")
    assert (info.bits_per_axis, info.fine_bits, F(info.cell_size)) == (g["bits"], g["fine"], g["h0"]), name
    assert info.n_reference == len(c["ref"])
    # (the order of the double additions is the device's own: the float mean may differ from numpy's in its last bit)
    assert (np.abs(h.reference_mean() - g["mean"]) <= np.spacing(np.abs(g["mean"]))).all(), (name, h.reference_mean(), g["mean"])


def _mean_frame(h, c):
    mean = h.reference_mean()
    ref_c = c["ref"].copy()
    ref_c[:, :3] -= mean
    T = synth.colmajor(c["T_init"]).copy()
    T[12:15] -= mean
    return mean, ref_c, T


def _extra_queries(ref_c, rng):
    """Uniform queries well outside the reference's box (between one and three extents from its centre on some axis), and
    queries on its six faces, its edges and corners among them."""
    lo, hi = ref_c[:, :3].min(0).astype(np.float64), ref_c[:, :3].max(0).astype(np.float64)
    mid, e = (lo + hi) / 2, max(float((hi - lo).max()), 1.0)
    out = mid + rng.uniform(-3 * e, 3 * e, (4000, 3))
    out = out[(np.abs(out - mid) > 1.0 * e).any(1)][:1000]
    face = rng.uniform(lo, hi, (640, 3))
    for i in range(len(face)):
        for d in range(3):
            if (i >> (2 * d)) & 3 == 1:
                face[i, d] = lo[d]
            elif (i >> (2 * d)) & 3 == 2:
                face[i, d] = hi[d]
    q = np.ones((len(out) + len(face), 4), F)
    q[:, :3] = np.concatenate([out, face]).astype(F)
    assert len(out) >= 500
    return q


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INTENDED))
def test_knn_matches_the_oracle(icp_mod, oracle, name):
    c = case(name)
    orc = _BruteOracle(oracle) if name in SEARCH_ONLY else oracle
    with icp_mod.IcpHandle(_config(c)) as h:
        h.set_reference(c["ref"], c["nrm"])
        _assert_geometry(h, c, name)
        _mean, ref_c, T = _mean_frame(h, c)
        ids, d2 = h.knn(c["rd"], T)                               # the reading under the guess
        _check_nn(orc, ref_c, oracle.transform_points(T, c["rd"]), ids, d2)
        q = _extra_queries(ref_c, np.random.default_rng(5))
        ids, d2 = h.knn(q, None)
        _check_nn(orc, ref_c, q, ids, d2)
        bi, bd = oracle.brute_nn(ref_c, q[::4])                   # ... and the brute force, independent of the tree
        assert np.array_equal(bd.view(np.uint32), d2[::4].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in INTENDED if n != "one_point"])
def test_knn_k_matches_the_brute_k_best(icp_mod, oracle, brute, name):
    c = case(name)
    with icp_mod.IcpHandle(_config(c)) as h:
        h.set_reference(c["ref"], None)
        _assert_geometry(h, c, name)
        _mean, ref_c, T = _mean_frame(h, c)
        rd = c["rd"][::2]
        q = np.concatenate([oracle.transform_points(T, rd), _extra_queries(ref_c, np.random.default_rng(6))[::2]])
        for k in (3, 8):
            ids, d2 = h.knn_k(q, k, None)
            bids, bd2 = brute(ref_c, q, k)
            _check_knn_k(ids, d2, bids, bd2, ref_c, q)
        ids, d2 = h.knn_k(rd, 3, T)                               # the transform applied by the search itself
        _check_knn_k(ids, d2, *brute(ref_c, q[:len(rd)], 3), ref_c, q[:len(rd)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in INTENDED if n != "one_point"])
def test_surface_normal_filter_equals_its_host_twin(icp_mod, name):
    """lsgpu_icp_filter_reference_normals (knn 10) == lsgpu_filter_surface_normal bit for bit: normals, ids, d2."""
    c = case(name)
    with icp_mod.IcpHandle(_config(c)) as h:
        dev = h.filter_reference_normals(c["ref"], 10, with_neighbours=True)
        _assert_geometry(h, c, name)                              # (the filter made the cloud the handle's reference)
        _same(dev, icp_mod.surface_normal(c["ref"], 10, with_neighbours=True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INTENDED))
def test_minimizer_sums_match_their_references(icp_mod, oracle, name):
    """lsgpu_normal_eq against oracle.point_to_plane and lsgpu_point_to_point against the numpy sums: the bars of
    test_normal_eq_matches_oracle and test_point_to_point_sums_match_numpy (relative, so they hold at any scale)."""
    c = case(name)
    with icp_mod.IcpHandle(_config(c)) as h:
        h.set_reference(c["ref"], c["nrm"])
        _assert_geometry(h, c, name)
        _mean, ref_c, T = _mean_frame(h, c)
        rd, rn = c["rd"], c["nrm"]
        ids, d2 = h.knn(rd, T)
        limit = h.trim_limit(d2, 0.75)
        A, b, used, _r2 = h.normal_eq(rd, T, ids, d2, limit)
        s = h.point_to_point(rd, T, ids, d2, limit)
    p = oracle.transform_points(T, rd)
    w = d2 <= F(limit)
    rc, Ao, bo, _xo, _dTo, used_o = oracle.point_to_plane(p, ref_c, rn, ids, d2, limit, 1)
    assert used == used_o == int(w.sum())
    print(name, "A", np.linalg.norm(A - Ao) / np.linalg.norm(Ao), "b", np.linalg.norm(b - bo) / max(np.linalg.norm(bo), 1e-300))
    assert np.linalg.norm(A - Ao) / np.linalg.norm(Ao) < 1e-12
    if np.linalg.norm(bo) > 0:
        assert np.linalg.norm(b - bo) / np.linalg.norm(bo) < 1e-10
    rc, Af, _bf, *_ = oracle.point_to_plane(p, ref_c, rn, ids, d2, limit, 0)
    assert np.linalg.norm(A - Af) / np.linalg.norm(Af) < 1e-5
    want = _sums(p[w, :3], ref_c[ids[w], :3])
    assert s[27] == want[27] == int(w.sum()) and (s[15:27] == 0).all()
    pd, qd = p[w, :3].astype(np.float64), ref_c[ids[w], :3].astype(np.float64)
    mag = np.concatenate([np.abs(pd).sum(0), np.abs(qd).sum(0), np.einsum("na,nc->ac", np.abs(qd), np.abs(pd)).ravel()])
    assert (np.abs(s[0:15] - want[0:15]) <= 1e-12 * mag).all()
    assert abs(s[28] - want[28]) <= 1e-12 * want[28]


def _in_mean_frame(T, m):
    """A transform between two clouds far from their frame's origin, conjugated into the reference-mean frame
    (t' = t + R m - m): there its lever arms are those of a sensor-frame cloud again."""
    T = np.asarray(T, np.float64).copy()
    T[:3, 3] = T[:3, 3] + T[:3, :3] @ m - m
    return T


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOOP_CASES)
def test_align_matches_the_oracle_loop(icp_mod, oracle, name):
    """The assertions of test_direction_index_on_clouds_it_is_not_made_for at the tightened checker: equal iteration
    count, per iteration the limit bit for bit, the inlier count, A to 1e-9; the pose within 1e-4 m / 1e-5 rad.  For a cloud
    scaled by s, min_diff_trans and the translation bar are scaled by s (the scaling is exact, so the oracle's run IS the
    scaled run); for far_origin both transforms are compared in the reference-mean frame."""
    from laser_slam_amd._lib import ConvergenceError
    c = case(name)
    s = c["scale"]
    ocfg = oracle.config_yaml(accum_double=1, min_diff_rot=1e-5, min_diff_trans=1e-4 * s)
    rc, To, sto, tro = oracle.icp_compute(ocfg, c["rd"], c["ref"], c["nrm"], synth.colmajor(c["T_init"]), 40)
    with icp_mod.IcpHandle(_config(c)) as h:
        h.set_reference(c["ref"], c["nrm"])
        _assert_geometry(h, c, name)
        if rc != 0:
            with pytest.raises(ConvergenceError):
                h.align(c["rd"], c["T_init"])
            return                                                # (test_the_oracle_converges_on_every_loop_case: not so today)
        Tg, stg = h.align(c["rd"], c["T_init"])
        trg = h.trace()
        mean = h.reference_mean().astype(np.float64)
    assert stg.iterations == sto.iterations and sto.iterations > 4, (name, stg.iterations, sto.iterations)
    for k, (a, b) in enumerate(zip(trg, tro)):
        assert F(a["limit"]) == F(b["limit"]), (name, k)
        assert a["n_used"] == b["n_used"], (name, k)
        assert np.linalg.norm(a["A"] - b["A"]) / np.linalg.norm(b["A"]) < 1e-9, (name, k)
    To4, Tg4 = synth.from_colmajor(To), Tg.astype(np.float64)
    if name == "far_origin":
        To4, Tg4 = _in_mean_frame(To4, mean), _in_mean_frame(Tg4, mean)
        assert stg.direction_index_launches == 0              # a cloud seen from far outside has no index by direction
    dt, dr = synth.pose_error(To4, Tg4)
    print(f"{name}: {stg.iterations} iterations, |dt| {dt:.3e} m (bar {TOL_T * s:.0e}), |dr| {dr:.3e} rad, "
          f"direction-index launches {stg.direction_index_launches}")
    assert dt <= TOL_T * s and dr <= TOL_R, (name, dt, dr)


CHAIN = dict(matcher=0.1, median=1.5)      # KDTreeMatcher maxDist 0.1 m + MedianDistOutlierFilter factor 1.5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["submap3", "stray"])
def test_chain_handle_matches_the_reference_loop(icp_mod, oracle, name):
    """One chain handle (a finite maxDist: the bounded k-best search; MedianDist: a quantile over the valid matches) on
    the 12-bit and the coarse-cell geometry, against the reference loop of test_outlier_chain."""
    c = case(name)
    Tg, st, trg, mean = _device_chain(icp_mod, c["ref"], c["nrm"], c["rd"], c["T_init"], 1, False, CHAIN)
    host, _ = host_chain_icp(oracle, _kd_nn(oracle), c["rd"], c["ref"], c["nrm"], c["T_init"], 1, CHAIN, mean=mean)
    assert host is not None
    facts = host[4]
    assert 0.05 <= facts[0]["invalid"] <= 0.60 and {f["binding"] for f in facts} == {"median"}, facts[0]   # both modules bite
    _compare_chain(Tg, st, trg, host)
    with icp_mod.IcpHandle(matcher_max_dist=CHAIN["matcher"], outlier_median_factor=CHAIN["median"]) as h:
        h.set_reference(c["ref"], c["nrm"])
        _assert_geometry(h, c, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCALE))
def test_scaling_by_a_power_of_two_scales_every_distance_exactly(icp_mod, name):
    """Metamorphic: d2 of the scaled pair is s^2 times d2 of the unscaled pair bit for bit (one neighbour and eight) --
    whatever the grid looks like, 11 bits for the one and 13 for the other."""
    c = case(name)
    s = F(c["scale"])
    _cloud, rf, rn, rd, T_init = _street()
    T1 = T_init.astype(F).astype(np.float64)
    with icp_mod.IcpHandle() as h1, icp_mod.IcpHandle(_config(c)) as hs:
        h1.set_reference(rf, rn)
        hs.set_reference(c["ref"], c["nrm"])
        _assert_geometry(hs, c, name)
        assert h1.info().bits_per_axis == 11 and np.array_equal(h1.reference_mean() * s, hs.reference_mean())
        _m, _r, Tm1 = _mean_frame(h1, dict(ref=rf, T_init=T1))
        _m, _r, Tms = _mean_frame(hs, c)
        assert np.array_equal(Tm1[12:15] * s, Tms[12:15]) and np.array_equal(Tm1[:12], Tms[:12])
        i1, d1 = h1.knn(rd, Tm1)
        i_s, d_s = hs.knn(c["rd"], Tms)
        assert np.array_equal((d1 * F(s * s)).view(np.uint32), d_s.view(np.uint32))
        assert (i1 != i_s).mean() < 0.01                        # (ties may go to another point at the same distance)
        _i1, k1 = h1.knn_k(rd[::4], 8, Tm1)
        _is, ks = hs.knn_k(c["rd"][::4], 8, Tms)
        assert np.array_equal((k1 * F(s * s)).view(np.uint32), ks.view(np.uint32))


@pytest.mark.gpu
def test_a_non_finite_reference_is_refused_and_leaves_a_usable_handle(icp_mod, pair4k):
    """A NaN or +-inf coordinate anywhere in the reference (first, middle, last point; nr not a multiple of 256):
    LSGPU_BAD_ARG, lsgpu_last_error names the cause, the handle has no reference afterwards, and the next valid
    set_reference + align give what a fresh handle gives, bit for bit."""
    from laser_slam_amd._lib import ConvergenceError, LsgpuError
    rf, rn = icp_mod.sampling_surface_normal(pair4k["ref"], 10, 1.0, 11)
    rf, rn = rf[:len(rf) - (len(rf) % 256) - 3], rn[:len(rf) - (len(rf) % 256) - 3]
    n = len(rf)
    assert n % 256 != 0 and n > 2000
    with icp_mod.IcpHandle() as fresh:
        fresh.set_reference(rf, rn)
        T0, st0 = fresh.align(pair4k["rd"], pair4k["T_init"])
        tr0 = [(t["limit"], t["n_used"], t["A"].tobytes()) for t in fresh.trace()]
    with icp_mod.IcpHandle() as h:
        for at, axis, v in [(0, 0, np.nan), (n // 2, 1, np.nan), (n - 1, 2, np.nan), (n // 3, 0, np.inf), (n - 1, 1, -np.inf),
                            (0, 2, np.inf)]:
            h.set_reference(rf, rn)                               # a good reference first: the refusal must drop it
            bad = rf.copy()
            bad[at, axis] = v
            with pytest.raises(LsgpuError) as e:
                h.set_reference(bad, rn)
            assert e.value.code == _lib.BAD_ARG and "non-finite" in str(e.value), (at, axis, v, str(e.value))
            with pytest.raises(ConvergenceError):                 # no reference == empty reference cloud
                h.align(pair4k["rd"], pair4k["T_init"])
            with pytest.raises(LsgpuError):
                h.info()
            h.set_reference(rf, rn)
            T1, st1 = h.align(pair4k["rd"], pair4k["T_init"])
            tr1 = [(t["limit"], t["n_used"], t["A"].tobytes()) for t in h.trace()]
            assert np.array_equal(T0, T1) and st0.iterations == st1.iterations and tr0 == tr1, (at, axis, v)
