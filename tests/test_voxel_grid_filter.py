"""VoxelGridDataPointsFilter of the input filter chain (include/lsgpu_icp.h, "the input filter chain"; DESIGN.md §5 choices
30-34): the host twin and the device path against a numpy float32 restatement of the contract written HERE, independent of
both.  Every comparison is bit for bit -- the contract fixes every rounding."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


class TooManyVoxels(Exception):
    pass


def ref_voxel_grid(pts, vsize, use_centroid):
    """The contract, restated: float32 throughout, one rounding per operation, a plain loop over the points in input order.
    Returns (output points (m, 4), first point's input index per output point, voxel index per output point)."""
    pts = np.ascontiguousarray(pts, np.float32)
    assert pts.shape[0] > 0 and np.isfinite(pts[:, :3]).all()
    v = [F(x) for x in vsize]
    minb, ndiv = [], []
    for a in range(3):
        mb = F(pts[:, a].min()) / v[a]
        xb = F(pts[:, a].max()) / v[a]
        t = (F(1.0) + xb) - mb
        if not t < F(2.0 ** 31):
            raise TooManyVoxels
        minb.append(mb)
        ndiv.append(max(int(t), 1))           # (uint) truncates; 0 (1 + maxB rounded to maxB) counts as 1
    if ndiv[0] * ndiv[1] * ndiv[2] > 2 ** 31 - 1:
        raise TooManyVoxels
    voxels = {}                               # voxel index -> [first, count, sx, sy, sz, (i, j, k)]; insertion order = first-point order
    for n in range(pts.shape[0]):
        c = []
        for a in range(3):
            c.append(min(int(np.floor(pts[n, a] / v[a] - minb[a])), ndiv[a] - 1))
        idx = c[0] + c[1] * ndiv[0] + c[2] * ndiv[0] * ndiv[1]
        vox = voxels.get(idx)
        if vox is None:
            voxels[idx] = [n, 1, pts[n, 0], pts[n, 1], pts[n, 2], c]
        else:
            vox[1] += 1
            vox[2] = vox[2] + pts[n, 0]       # np.float32 scalars: each addition rounds once
            vox[3] = vox[3] + pts[n, 1]
            vox[4] = vox[4] + pts[n, 2]
    out = np.empty((len(voxels), 4), np.float32)
    for o, (first, count, sx, sy, sz, c) in enumerate(voxels.values()):
        if use_centroid:
            out[o, 0], out[o, 1], out[o, 2] = sx / F(count), sy / F(count), sz / F(count)
        else:
            for a in range(3):
                out[o, a] = v[a] * ((minb[a] + F(c[a])) + F(0.5))
        out[o, 3] = pts[first, 3]
    return out, np.array([vx[0] for vx in voxels.values()], np.int64), np.array(list(voxels.keys()), np.int64)


def _indexed(xyz):
    """(n, 3) -> x, y, z, w with w = the point's index as a float (case 6: the fourth component travels with the first point)."""
    p = np.empty((xyz.shape[0], 4), np.float32)
    p[:, :3] = xyz
    p[:, 3] = np.arange(xyz.shape[0], dtype=np.float32)
    return p


def _scan(n_az=64, noise_seed=70):
    return _indexed(synth.hdl64_scan(synth.Scene(1234), synth.se3(0.0, 0.0, synth.SENSOR_HEIGHT), n_az, noise_seed)[:, :3])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, vSize, useCentroid, reference output, first indices, voxel indices); computed once, never changed."""
    rng = np.random.default_rng(11)
    scan = _scan()
    assert 3000 < scan.shape[0] < 5000 and (scan[:, :3].min(0) < 0).all() and (scan[:, :3].max(0) > 0).all()
    lattice = np.array([(i, j, k) for i in range(-3, 4) for j in range(-3, 4) for k in range(-2, 4)], np.float32)
    lattice = lattice[rng.permutation(lattice.shape[0])[:257]]              # spacing 1 = 2 vSize: one point per voxel
    desc = np.arange(40, dtype=np.float32)[::-1].reshape(-1, 1) * np.array([[0.75, 0.0, 0.0]], np.float32)   # x = 29.25 ... 0
    desc = np.concatenate([desc, desc + np.array([[0.1, 0.1, 0.1]], np.float32)], 0)                          # a second point per voxel
    same = np.tile(np.array([[1.3, -2.7, 0.4]], np.float32), (100, 1))
    todo = {
        "scan_centroid": (scan, (0.5, 0.5, 0.5), 1),
        "scan_centre": (scan, (0.5, 1.0, 2.0), 0),
        "scan_fine": (scan, (0.05, 0.05, 0.05), 1),                         # > 2^24 voxels: four passes of the sort
        "one_voxel": (_indexed(rng.uniform(10.0, 10.9, (3000, 3)).astype(np.float32)), (1.0, 1.0, 1.0), 1),
        "lattice": (_indexed(lattice), (0.5, 0.5, 0.5), 1),
        "descending": (_indexed(desc), (0.75, 0.75, 0.75), 1),
        "single": (_indexed(np.array([[-4.5, 2.25, 0.125]], np.float32)), (1.0, 1.0, 1.0), 1),
        "identical": (_indexed(same), (0.3, 0.3, 0.3), 1),
        "identical_centre": (_indexed(same), (0.3, 0.3, 0.3), 0),
    }
    out = {}
    for name, (pts, vs, uc) in todo.items():
        pts.setflags(write=False)
        want, first, vox = ref_voxel_grid(pts, vs, uc)
        for a in (want, first, vox):
            a.setflags(write=False)
        out[name] = (pts, vs, uc, want, first, vox)
    return out


CASE_NAMES = ["scan_centroid", "scan_centre", "scan_fine", "one_voxel", "lattice", "descending", "single", "identical", "identical_centre"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _spec(vsize, use_centroid=1, average=1):
    return (_lib.FILTER_VOXEL_GRID, average, use_centroid, list(vsize))


def _chain(mod, specs):
    arr = (mod.PointFilter * len(specs))()
    for a, (typ, dim, flag, v) in zip(arr, specs):
        a.type, a.dim, a.flag = typ, dim, flag
        for i, x in enumerate(v):
            a.v[i] = x
        a.state = 0.0
    return arr


# ---------------------------------------------------------------- CPU: the host twin against the restatement

@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_twin_matches_restatement(name):
    from laser_slam_amd import icp
    pts, vs, uc, want, first, _ = cases()[name]
    got = icp.voxel_grid_points(pts, vs, uc)
    assert _same(got, want), name
    assert np.array_equal(got[:, 3], first.astype(np.float32))              # the fourth component is the first point's


def test_restatement_properties():
    """What the cases are there for, judged on the restatement itself (the host twin and the device are compared with it)."""
    c = cases()
    assert c["one_voxel"][3].shape[0] == 1 and c["one_voxel"][0].shape[0] == 3000      # one run longer than a 256-thread block
    pts, _, _, want, first, vox = c["lattice"]
    assert _same(want, pts) and np.array_equal(first, np.arange(257))                  # one point per voxel: the input, order included
    pts, _, _, want, first, vox = c["descending"]
    assert want.shape[0] == 40 and np.array_equal(first, np.arange(40))                # first-point order ...
    assert (np.diff(vox) < 0).all() and not np.array_equal(np.argsort(vox), np.arange(40))   # ... which is NOT voxel-index order
    assert (np.diff(want[:, 0]) < 0).all()
    assert c["single"][3].shape[0] == 1 and _same(c["single"][3], c["single"][0])
    assert c["identical"][3].shape[0] == 1 and c["identical"][3][0, 3] == 0.0
    for name in ("scan_centroid", "scan_centre", "scan_fine"):
        pts, _, _, want, first, vox = c[name]
        assert 1 < want.shape[0] < pts.shape[0] and (np.diff(first) > 0).all() and len(set(vox.tolist())) == len(vox)
    assert not (np.diff(c["scan_centroid"][5]) > 0).all()                               # the scan's voxels are not in index order either
    assert c["scan_fine"][5].max() >= 1 << 24


def test_host_twin_refusals():
    from laser_slam_amd import icp
    rng = np.random.default_rng(3)
    big = _indexed(rng.uniform(-50.0, 50.0, (500, 3)).astype(np.float32))
    with pytest.raises(TooManyVoxels):
        ref_voxel_grid(big, (1e-4, 1e-4, 1e-4), 1)
    dirty = big.copy()
    dirty[17, 1] = np.nan
    for pts, vs, uc, code in ((big, (1e-4, 1e-4, 1e-4), 1, _lib.BAD_CONFIG), (dirty, (0.5, 0.5, 0.5), 1, _lib.BAD_ARG),
                              (big, (0.0, 0.5, 0.5), 1, _lib.BAD_CONFIG), (big, (0.5, -1.0, 0.5), 1, _lib.BAD_CONFIG),
                              (big, (0.5, 0.5, np.inf), 1, _lib.BAD_CONFIG), (big, (0.5, 0.5, 0.5), 2, _lib.BAD_CONFIG)):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.voxel_grid_points(pts, vs, uc)
        assert e.value.code == code, (vs, uc)
    with pytest.raises(_lib.ConvergenceError):
        icp.voxel_grid_points(big[:0], (0.5, 0.5, 0.5), 1)
    assert _lib.lib().lsgpu_abi_version() == 4 and _lib.FILTER_VOXEL_GRID == 7


@pytest.fixture(scope="module")
def facade_check(tmp_path_factory):
    """tests/cpp/voxel_filter_check.cpp, built once: files -> what DataPointsFilters / the shim / LaserTrack make of them."""
    exe = str(tmp_path_factory.mktemp("voxel_filter_check") / "voxel_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "cpp", "voxel_filter_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])

    def run(*paths):
        r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "DESCRIPTOR_RULE throws throws" in r.stdout, r.stdout + r.stderr
        files, cur = [], None
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "FILE":
                cur = dict(modules=[], error=None, shim=None, track=None)
                files.append(cur)
            elif w[0] == "MODULE":
                cur["modules"].append((int(w[1]), int(w[2]), int(w[3]), [np.float32(x) for x in w[4:10]]))
            elif w[0] == "CONFIG_ERROR":
                cur["error"] = line
            elif w[0] == "SHIM":
                cur["shim"] = (int(w[1]), w[2])
            elif w[0] == "TRACK":
                cur["track"] = int(w[1])
        return files
    return run


def test_cpp_facade_parses_the_module(facade_check, tmp_path):
    docs = {
        "defaults": "- VoxelGridDataPointsFilter\n",
        "values": "- RemoveNaNDataPointsFilter\n- VoxelGridDataPointsFilter:\n    vSizeX: 0.1\n    vSizeY: 0.25\n    vSizeZ: 3\n"
                  "    useCentroid: 0\n    averageExistingDescriptors: 0\n",
        "unknown": "- VoxelGridDataPointsFilter: {vSizeX: 0.5, vSize: 1}\n",
        "zero": "- VoxelGridDataPointsFilter: {vSizeY: 0}\n",
        "inf": "- VoxelGridDataPointsFilter: {vSizeZ: inf}\n",
        "flag": "- VoxelGridDataPointsFilter: {useCentroid: 2}\n",
    }
    for k, text in docs.items():
        (tmp_path / (k + ".yaml")).write_text(text)
    res = dict(zip(docs, facade_check(*[tmp_path / (k + ".yaml") for k in docs])))
    d = res["defaults"]
    assert d["error"] is None and d["modules"] == [(7, 1, 1, [F(1), F(1), F(1), F(0), F(0), F(0)])]     # (1, 1, 1, 1, 1)
    assert d["shim"] == (1, "same") and d["track"] == 1                    # the shim and LaserTrack load such a file
    v = res["values"]
    assert v["error"] is None and v["modules"][0][0] == _lib.FILTER_REMOVE_NAN
    assert v["modules"][1] == (7, 0, 0, [F(0.1), F(0.25), F(3), F(0), F(0), F(0)]) and v["shim"] == (2, "same") and v["track"] == 2
    assert "unknown parameter vSize" in res["unknown"]["error"] and not res["unknown"]["modules"]
    for k in ("zero", "inf", "flag"):
        assert res[k]["error"] and "VoxelGridDataPointsFilter" in res[k]["error"], k


def test_upstream_dump_writes_the_module(facade_check, tmp_path, oracle):
    spec = importlib.util.spec_from_file_location("dump_for_upstream", os.path.join(ROOT, "devtools", "dump_for_upstream.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (tmp_path / "one.yaml").write_text(mod.voxel_grid_yaml((0.1, 1.0 / 3.0, 2.5), 0, 0))
    flt = mod.input_chain_for_dump(str(tmp_path), [0.3, 0.4, 0.7, 1])      # the golden chain + the module -> input_filters.yaml
    one, chain = facade_check(tmp_path / "one.yaml", tmp_path / "input_filters.yaml")
    assert one["error"] is None and one["modules"] == [(7, 0, 0, [F(0.1), F(1.0 / 3.0), F(2.5), F(0), F(0), F(0)])]
    assert chain["error"] is None and len(chain["modules"]) == len(flt) == 6
    for got, a in zip(chain["modules"], flt):                              # the facade's descriptor == the one the tool runs
        assert got == (a.type, a.dim, a.flag, [F(a.v[i]) for i in range(6)])
    assert chain["modules"][5][:3] == (7, 0, 1)
    # ... and the tool's run of that chain is the oracle's run of the golden chain followed by the restatement
    scan = _scan()
    golden = mod.input_filter_chain(os.path.join(ROOT, "tests", "golden", "input_filters.yaml"))
    want, _, _ = ref_voxel_grid(oracle.apply_point_filters(golden, scan, seed=1), (F(0.3), F(0.4), F(0.7)), 1)
    assert _same(mod.run_input_filters(flt, scan, 1), want)


# ---------------------------------------------------------------- GPU: through lsgpu_apply_point_filters

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_matches_host_twin_and_restatement(name):
    import torch
    from laser_slam_amd import icp
    pts, vs, uc, want, first, _ = cases()[name]
    twin = icp.voxel_grid_points(pts, vs, uc)
    with icp.IcpHandle() as h:
        got = h.apply_point_filters(_chain(_lib, [_spec(vs, uc)]), pts)                       # host in, host out
        assert _same(got, want) and _same(got, twin), name
        dev = h.apply_point_filters(_chain(_lib, [_spec(vs, uc, 0)]), torch.from_numpy(np.array(pts)).cuda())   # device in, device out
        assert dev.is_cuda and _same(dev.cpu().numpy(), want), name


@pytest.mark.gpu
def test_chain_continues_the_draw_stream(oracle):
    """[MaxDist 30 radial, VoxelGrid 0.5, RandomSampling 0.5], seed 7 == the three steps one by one: the module consumes no
    draw and the next module draws once per OUTPUT point."""
    from laser_slam_amd import icp
    scan = _scan()
    specs = [(_lib.FILTER_MAX_DIST, -1, 0, [30.0]), _spec((0.5, 0.5, 0.5)), (_lib.FILTER_RANDOM_SAMPLING, 0, 0, [0.5])]
    a = oracle.apply_point_filters(_chain(oracle, specs[:1]), scan, seed=7)
    b, _, _ = ref_voxel_grid(a, (0.5, 0.5, 0.5), 1)
    want = oracle.apply_point_filters(_chain(oracle, specs[2:]), b, seed=-1)
    assert 0 < want.shape[0] < b.shape[0] < a.shape[0] < scan.shape[0]
    with icp.IcpHandle() as h:
        got = h.apply_point_filters(_chain(_lib, specs), scan, seed=7)
    assert _same(got, want)


@pytest.mark.gpu
def test_one_descriptor_array_two_scans():
    """Buffer reuse on one handle: the same descriptor array on a scan and then on a larger one."""
    from laser_slam_amd import icp
    small, large = _scan(32, 5), _scan(64, 6)
    assert small.shape[0] < large.shape[0]
    chain = _chain(_lib, [_spec((0.4, 0.4, 0.4))])
    with icp.IcpHandle() as h:
        for s in (small, large, small):
            assert _same(h.apply_point_filters(chain, s), ref_voxel_grid(s, (0.4, 0.4, 0.4), 1)[0])


@pytest.mark.gpu
def test_device_refusals_leave_the_handle_usable():
    """Ordinary bad arguments: refused by the validation loop before any launch, or after the bounds pass."""
    from laser_slam_amd import icp
    rng = np.random.default_rng(3)
    big = _indexed(rng.uniform(-50.0, 50.0, (500, 3)).astype(np.float32))
    dirty = big.copy()
    dirty[17, 1] = np.nan
    inf = big.copy()
    inf[3, 2] = -np.inf
    L = _lib.lib()
    with icp.IcpHandle() as h:
        for pts, spec, code, word in ((big, _spec((1e-4, 1e-4, 1e-4)), _lib.BAD_CONFIG, "too many voxels"),
                                      (dirty, _spec((0.5, 0.5, 0.5)), _lib.BAD_ARG, "RemoveNaNDataPointsFilter"),
                                      (inf, _spec((0.5, 0.5, 0.5)), _lib.BAD_ARG, "RemoveNaNDataPointsFilter"),
                                      (big, _spec((0.0, 0.5, 0.5)), _lib.BAD_CONFIG, "vSize"),
                                      (big, _spec((0.5, -1.0, 0.5)), _lib.BAD_CONFIG, "vSize"),
                                      (big, _spec((0.5, 0.5, np.inf)), _lib.BAD_CONFIG, "vSize"),
                                      (big, _spec((0.5, 0.5, 0.5), 2), _lib.BAD_CONFIG, "useCentroid"),
                                      (big, _spec((0.5, 0.5, 0.5), 1, 2), _lib.BAD_CONFIG, "averageExistingDescriptors")):
            with pytest.raises(_lib.LsgpuError) as e:
                h.apply_point_filters(_chain(_lib, [spec]), pts)
            assert e.value.code == code and word in L.lsgpu_last_error(h._h).decode(), spec
        # a bad parameter anywhere in the chain is refused before anything runs: no draw is consumed, nothing is written
        with pytest.raises(_lib.LsgpuError) as e:
            h.apply_point_filters(_chain(_lib, [(_lib.FILTER_RANDOM_SAMPLING, 0, 0, [0.5]), _spec((0.5, 0.5, 0.0))]), big, seed=3)
        assert e.value.code == _lib.BAD_CONFIG
        pts, vs, uc, want, _, _ = cases()["scan_centroid"]
        assert _same(h.apply_point_filters(_chain(_lib, [_spec(vs, uc)]), pts), want)


@pytest.mark.gpu
def test_empty_cloud_mid_chain():
    from laser_slam_amd import icp
    scan = _scan()
    with icp.IcpHandle() as h:
        with pytest.raises(_lib.ConvergenceError):
            h.apply_point_filters(_chain(_lib, [(_lib.FILTER_MAX_DIST, -1, 0, [0.001]), _spec((0.5, 0.5, 0.5))]), scan)
        got = h.apply_point_filters(_chain(_lib, [_spec((0.5, 0.5, 0.5)), (_lib.FILTER_MAX_DIST, -1, 0, [0.001])]), scan)
        assert got.shape[0] == 0                                             # (the last module may empty the cloud)
