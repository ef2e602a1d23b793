"""OctreeGridDataPointsFilter of the input filter chain (include/lsgpu_icp.h, "the input filter chain"; DESIGN.md §5 choices
49-54): the host twin against tests/octree_model.py -- a numpy float32 recursion of the contract, independent of the library
-- and the device path against the host twin.  Every comparison is bit for bit: the contract fixes every rounding.  The draws
of RandomPts are glibc's srand / rand sequence, taken from libc itself."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import octree_model as M
import prim_cases as P
from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
METHODS = (M.FIRST_PTS, M.RANDOM_PTS, M.CENTROID, M.MEDOID)
KEY_BLOCK = 256                                  # k_ogf_keys' block
SORT_TILE = 256 * 4                              # keys per block of the sort under ITEMS 4
SORT_CHUNK = SORT_TILE * P.RS_CHUNK              # pairs per chunk of k_rs_scan under ITEMS 4
SEED = 5


def libc_draws(seed, skip, n):
    """draws skip + 1 .. skip + n of std::srand(seed) + (float)std::rand() / (float)RAND_MAX"""
    libc = C.CDLL("libc.so.6")
    libc.rand.restype = C.c_int
    libc.srand(C.c_uint(seed))
    r = np.array([libc.rand() for _ in range(skip + n)], np.int64)[skip:]
    return r.astype(np.float32) / np.float32(2147483648.0)


def _indexed(xyz):
    """(n, 3) -> x, y, z, w with w = the point's index as a float: which input point an output point is shows in w"""
    p = np.empty((xyz.shape[0], 4), np.float32)
    p[:, :3] = xyz
    p[:, 3] = np.arange(xyz.shape[0], dtype=np.float32)
    return p


def _scan(n_az=64, noise_seed=70):
    return _indexed(synth.hdl64_scan(synth.Scene(1234), synth.se3(0.0, 0.0, synth.SENSOR_HEIGHT), n_az, noise_seed)[:, :3])


def _uniform(rng, n, lo=-20.0, hi=20.0):
    return _indexed(rng.uniform(lo, hi, (n, 3)).astype(np.float32))


class Case:
    def __init__(self, pts, max_size, max_point):
        pts.setflags(write=False)
        self.pts, self.max_size, self.max_point = pts, max_size, max_point
        self._out = {}
        _, self.leaves = M.octree_grid(pts, max_size, max_point, M.FIRST_PTS)

    def want(self, method):
        """The model's output (computed once, never changed); RandomPts with the draws 1 .. n_leaves of srand(SEED)"""
        if method not in self._out:
            draws = libc_draws(SEED, 0, len(self.leaves)) if method == M.RANDOM_PTS else None
            out, leaves = M.octree_grid(self.pts, self.max_size, self.max_point, method, draws)
            out.setflags(write=False)
            self._out[method] = (out, leaves)
        return self._out[method][0]

    def ties(self):
        self.want(M.MEDOID)
        return sum(1 for leaf in self._out[M.MEDOID][1] if leaf.tie)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(23)
    scan = _scan()
    assert 3000 < scan.shape[0] < 5000
    same = np.tile(np.array([[1.3, -2.7, 0.4]], np.float32), (100, 1))
    planar = rng.uniform(-5.0, 5.0, (500, 3)).astype(np.float32)
    planar[:, 2] = F(0.75)
    dup = rng.uniform(-3.0, 3.0, (300, 3)).astype(np.float32)
    dup[[5, 17, 40, 41, 99, 100, 150, 222, 250, 299]] = dup[5]          # ten copies of one point, scattered over the input
    dup[[7, 8, 200]] = dup[7]                                           # and three of another
    pairs = np.array([[0, 0, 0], [2, 0, 0], [10, 10, 10], [12, 10, 10], [0, 8, 0], [0, 8, 4]], np.float32)
    box = rng.uniform(0.0, 8.0, (3000, 3)).astype(np.float32)
    box[0], box[1] = (0.0, 0.0, 0.0), (8.0, 8.0, 8.0)                   # the extent is exactly 8: radius 4, 2, 1 ...
    return {
        "single": Case(_indexed(np.array([[-4.5, 2.25, 0.125]], np.float32)), 0.0, 1),
        "two_identical": Case(_indexed(same[:2]), 0.0, 1),
        "identical": Case(_indexed(same), 0.0, 7),
        "planar": Case(_indexed(planar), 0.0, 1),
        "key_block": Case(_uniform(rng, KEY_BLOCK), 0.0, 1),
        "key_block_1": Case(_uniform(rng, KEY_BLOCK + 1), 0.0, 1),
        "sort_tile": Case(_uniform(rng, SORT_TILE), 0.0, 7),
        "sort_tile_1": Case(_uniform(rng, SORT_TILE + 1), 0.0, 7),
        "sort_chunk": Case(_uniform(rng, SORT_CHUNK), 0.0, 64),
        "sort_chunk_1": Case(_uniform(rng, SORT_CHUNK + 1), 0.0, 64),
        "duplicates_p1": Case(_indexed(dup), 0.0, 1),
        "duplicates_p7": Case(_indexed(dup), 0.0, 7),
        "medoid_tie": Case(_indexed(pairs), 0.0, 2),
        "long_leaves": Case(_indexed(box), 4.0, 7),
        "one_leaf": Case(_indexed(box), 100.0, 1),
        "scan_p1": Case(scan, 0.0, 1),
        "scan_p7_size": Case(scan, 0.5, 7),
        "scan_p64": Case(scan, 0.0, 64),
    }


CASE_NAMES = ["single", "two_identical", "identical", "planar", "key_block", "key_block_1", "sort_tile", "sort_tile_1", "sort_chunk",
              "sort_chunk_1", "duplicates_p1", "duplicates_p7", "medoid_tie", "long_leaves", "one_leaf", "scan_p1", "scan_p7_size",
              "scan_p64"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _spec(max_size=0.0, max_point=1, method=0, build_parallel=1):
    return (_lib.FILTER_OCTREE_GRID, method, build_parallel, [max_size, max_point])


def _chain(mod, specs):
    arr = (mod.PointFilter * len(specs))()
    for a, (typ, dim, flag, v) in zip(arr, specs):
        a.type, a.dim, a.flag = typ, dim, flag
        for i, x in enumerate(v):
            a.v[i] = x
        a.state = 0.0
    return arr


# ---------------------------------------------------------------- CPU: the model, the cases, the host twin

def test_model_sums_one_point_after_the_other():
    """np.add.accumulate, which the model's centroid uses, is the plain loop of the contract"""
    v = np.random.default_rng(1).uniform(-100.0, 100.0, (3001, 3)).astype(np.float32)
    acc = np.add.accumulate(v, axis=0, dtype=np.float32)[-1]
    for a in range(3):
        assert acc[a].view(np.uint32) == M.sequential_sum(v[:, a]).view(np.uint32)
    pairwise = np.array([np.ascontiguousarray(v[:, a]).sum(dtype=np.float32) for a in range(3)])
    assert not np.array_equal(acc, pairwise)                               # (numpy's blocked sum is NOT it: the order matters)


def test_cases_have_the_properties_they_are_there_for():
    """Conditions on the inputs, judged on the model's leaves (the host twin and the device are compared with its output)."""
    assert SORT_TILE == 1024 and SORT_CHUNK == 262144 and SORT_CHUNK in P.SORT_SIZES and SORT_CHUNK + 1 in P.SORT_SIZES
    assert P.sort_shape(SORT_TILE)["blocks"] == 1 and P.sort_shape(SORT_TILE + 1)["blocks"] == 2
    assert P.sort_shape(SORT_CHUNK)["chunks"] == 1 and P.sort_shape(SORT_CHUNK + 1)["chunks"] == 2
    c = cases()
    assert sorted(c) == sorted(CASE_NAMES)
    for name, case in c.items():                                           # every point is in exactly one leaf, in ascending index
        idx = np.concatenate([leaf.idx for leaf in case.leaves])
        assert np.array_equal(np.sort(idx), np.arange(case.pts.shape[0])), name
        assert all((np.diff(leaf.idx) > 0).all() for leaf in case.leaves), name
        assert all(leaf.depth <= M.MAX_DEPTH for leaf in case.leaves), name
    assert len(c["single"].leaves) == 1 and c["single"].leaves[0].depth == 0
    for name, count in (("two_identical", 2), ("identical", 100)):          # radius 0: the root is a size-stopped leaf
        (leaf,) = c[name].leaves
        assert leaf.why == "size" and leaf.radius == 0 and leaf.idx.size == count > c[name].max_point
    assert np.ptp(c["planar"].pts[:, 2]) == 0 and len(c["planar"].leaves) == 500
    for name, n in (("key_block", KEY_BLOCK), ("key_block_1", KEY_BLOCK + 1), ("sort_tile", SORT_TILE), ("sort_tile_1", SORT_TILE + 1),
                    ("sort_chunk", SORT_CHUNK), ("sort_chunk_1", SORT_CHUNK + 1)):
        assert c[name].pts.shape[0] == n and 1 < len(c[name].leaves) <= n
        assert all(leaf.why == "count" for leaf in c[name].leaves), name
    sizes = {leaf.idx.size for leaf in c["sort_chunk"].leaves}                          # short and long leaves side by side
    assert min(sizes) <= 4 and 48 <= max(sizes) <= 64 and len(sizes) >= 32
    # more than maxPointByNode exact duplicates: a leaf at the depth cap that holds them all, scattered input indices
    deep = [leaf for leaf in c["duplicates_p1"].leaves if leaf.why == "depth"]
    assert sorted(leaf.idx.size for leaf in deep) == [3, 10] and all(leaf.depth == 21 for leaf in deep)
    deep = [leaf for leaf in c["duplicates_p7"].leaves if leaf.why == "depth"]
    assert [leaf.idx.size for leaf in deep] == [10] and deep[0].depth == 21 and deep[0].idx.tolist() == [5, 17, 40, 41, 99, 100, 150, 222, 250, 299]
    assert any(leaf.why == "count" and {7, 8, 200} <= set(leaf.idx.tolist()) for leaf in c["duplicates_p7"].leaves)   # (three fit a leaf of 7)
    assert c["medoid_tie"].ties() == 3 and [leaf.idx.tolist() for leaf in c["medoid_tie"].leaves] == [[0, 1], [4, 5], [2, 3]]
    assert _same(c["medoid_tie"].want(M.MEDOID), c["medoid_tie"].pts[[0, 4, 2]])     # the earliest wins
    long_leaves = c["long_leaves"].leaves
    assert len(long_leaves) == 8 and all(leaf.why == "size" and leaf.depth == 1 and leaf.idx.size > 256 for leaf in long_leaves)
    (leaf,) = c["one_leaf"].leaves
    assert leaf.why == "size" and leaf.depth == 0 and leaf.idx.size == 3000
    for name in ("scan_p1", "scan_p7_size", "scan_p64"):
        n_leaves, n = len(c[name].leaves), c[name].pts.shape[0]
        assert 1 < n_leaves < n or (name == "scan_p1" and n_leaves == n), name
    assert len(c["scan_p64"].leaves) < len(c["scan_p7_size"].leaves) < len(c["scan_p1"].leaves)
    sized = [leaf for leaf in c["scan_p7_size"].leaves if leaf.why == "size"]
    assert sized and max(leaf.idx.size for leaf in sized) > 7 and any(leaf.why == "count" for leaf in c["scan_p7_size"].leaves)
    # the leaf order is NOT input order, and RandomPts does not always take the first point
    first = c["scan_p7_size"].want(M.FIRST_PTS)[:, 3]
    assert not (np.diff(first) > 0).all()
    assert not np.array_equal(c["scan_p7_size"].want(M.RANDOM_PTS)[:, 3], first)
    assert not _same(c["scan_p7_size"].want(M.MEDOID), c["scan_p7_size"].want(M.FIRST_PTS))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_twin_matches_model(name):
    from laser_slam_amd import icp
    case = cases()[name]
    for method in METHODS:
        got = icp.octree_grid_points(case.pts, case.max_size, case.max_point, method, SEED)
        assert _same(got, case.want(method)), (name, method)


def test_host_twin_continues_the_draw_stream():
    """RandomPts takes exactly one draw per leaf: what follows it on the stream are the next draws"""
    from laser_slam_amd import icp
    case = cases()["scan_p7_size"]
    n_leaves = len(case.leaves)
    assert _same(icp.octree_grid_points(case.pts, case.max_size, case.max_point, M.RANDOM_PTS, SEED), case.want(M.RANDOM_PTS))
    keep = icp.random_sampling(2000, 0.5, -1)
    assert np.array_equal(keep, np.nonzero(libc_draws(SEED, n_leaves, 2000) < F(0.5))[0])
    for method in (M.FIRST_PTS, M.CENTROID, M.MEDOID):                     # ... and the other methods take none
        icp.random_sampling(0, 0.5, SEED)
        icp.octree_grid_points(case.pts, case.max_size, case.max_point, method, -1)
        assert np.array_equal(icp.random_sampling(2000, 0.5, -1), np.nonzero(libc_draws(SEED, 0, 2000) < F(0.5))[0])


def test_host_twin_refusals():
    from laser_slam_amd import icp
    big = _uniform(np.random.default_rng(3), 500)
    dirty = big.copy()
    dirty[17, 1] = np.nan
    inf = big.copy()
    inf[3, 2] = -np.inf
    for pts, args, code in ((dirty, (0.0, 1, 0), _lib.BAD_ARG), (inf, (0.0, 1, 0), _lib.BAD_ARG),
                            (big, (-1.0, 1, 0), _lib.BAD_CONFIG), (big, (np.inf, 1, 0), _lib.BAD_CONFIG), (big, (np.nan, 1, 0), _lib.BAD_CONFIG),
                            (big, (0.0, 0, 0), _lib.BAD_CONFIG), (big, (0.0, -3, 0), _lib.BAD_CONFIG), (big, (0.0, 2 ** 24 + 1, 0), _lib.BAD_CONFIG),
                            (big, (0.0, 1, 4), _lib.BAD_CONFIG), (big, (0.0, 1, -1), _lib.BAD_CONFIG)):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.octree_grid_points(pts, *args)
        assert e.value.code == code, args
    with pytest.raises(_lib.ConvergenceError):
        icp.octree_grid_points(big[:0])
    assert icp.octree_grid_points(big, 0.0, 2 ** 24).shape[0] == 1             # the largest maxPointByNode
    assert _lib.lib().lsgpu_abi_version() == 4 and _lib.FILTER_OCTREE_GRID == 8 and C.sizeof(_lib.PointFilter) == 48


@pytest.fixture(scope="module")
def facade_check(tmp_path_factory):
    """tests/cpp/octree_filter_check.cpp, built once: files -> what DataPointsFilters / the shim / LaserTrack make of them."""
    exe = str(tmp_path_factory.mktemp("octree_filter_check") / "octree_filter_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "cpp", "octree_filter_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])

    def run(*paths):
        r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "DESCRIPTOR_RULE throws throws passes passes" in r.stdout, r.stdout + r.stderr
        files, cur = [], None
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "FILE":
                cur = dict(modules=[], error=None, shim=None, shim_error=None, track=None, track_error=None)
                files.append(cur)
            elif w[0] == "MODULE":
                cur["modules"].append((int(w[1]), int(w[2]), int(w[3]), [np.float32(x) for x in w[4:10]]))
            elif w[0] == "CONFIG_ERROR":
                cur["error"] = line
            elif w[0] == "SHIM":
                cur["shim"] = (int(w[1]), w[2])
            elif w[0] == "SHIM_ERROR":
                cur["shim_error"] = line
            elif w[0] == "TRACK":
                cur["track"] = int(w[1])
            elif w[0] == "TRACK_ERROR":
                cur["track_error"] = line
        return files
    return run


def test_cpp_facade_parses_the_module(facade_check, tmp_path):
    docs = {
        "defaults": "- OctreeGridDataPointsFilter\n",
        "values": "- RemoveNaNDataPointsFilter\n- OctreeGridDataPointsFilter:\n    buildParallel: 0\n    maxPointByNode: 64\n"
                  "    maxSizeByNode: 0.25\n    samplingMethod: 3\n",
        "inline": "- OctreeGridDataPointsFilter: {maxSizeByNode: 0.1, samplingMethod: 1}\n",
        "unknown": "- OctreeGridDataPointsFilter: {maxSizeByNode: 0.5, maxSize: 1}\n",
        "points": "- OctreeGridDataPointsFilter: {maxPointByNode: 0}\n",
        "fraction": "- OctreeGridDataPointsFilter: {maxPointByNode: 2.5}\n",
        "size": "- OctreeGridDataPointsFilter: {maxSizeByNode: -1}\n",
        "method": "- OctreeGridDataPointsFilter: {samplingMethod: 4}\n",
        "parallel": "- OctreeGridDataPointsFilter: {buildParallel: 2}\n",
    }
    for k, text in docs.items():
        (tmp_path / (k + ".yaml")).write_text(text)
    res = dict(zip(docs, facade_check(*[tmp_path / (k + ".yaml") for k in docs])))
    zero = [F(0)] * 4
    d = res["defaults"]
    assert d["error"] is None and d["modules"] == [(8, 0, 1, [F(0), F(1)] + zero)]     # maxSizeByNode 0, maxPointByNode 1, FirstPts, parallel
    assert d["shim"] == (1, "same") and d["track"] == 1                                # the shim and LaserTrack load such a file
    v = res["values"]
    assert v["error"] is None and v["modules"][0][0] == _lib.FILTER_REMOVE_NAN
    assert v["modules"][1] == (8, 3, 0, [F(0.25), F(64)] + zero) and v["shim"] == (2, "same") and v["track"] == 2
    assert res["inline"]["modules"] == [(8, 1, 1, [F(0.1), F(1)] + zero)] and res["inline"]["track"] == 1
    assert "unknown parameter maxSize" in res["unknown"]["error"] and not res["unknown"]["modules"]
    for k, word in (("unknown", "maxSize"), ("points", "maxPointByNode"), ("fraction", "maxPointByNode"), ("size", "maxSizeByNode"),
                    ("method", "samplingMethod"), ("parallel", "buildParallel")):
        for who in ("error", "shim_error", "track_error"):                             # all three refuse, module and parameter named
            assert res[k][who] and "OctreeGridDataPointsFilter" in res[k][who] and word in res[k][who], (k, who)
        assert res[k]["shim"] is None and res[k]["track"] is None


def _dump_tool():
    spec = importlib.util.spec_from_file_location("dump_for_upstream", os.path.join(ROOT, "devtools", "dump_for_upstream.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_upstream_dump_writes_the_module(facade_check, tmp_path, oracle):
    mod = _dump_tool()
    (tmp_path / "one.yaml").write_text(mod.octree_grid_yaml(1.0 / 3.0, 7, 3, 0))
    with pytest.raises(SystemExit):                                        # RandomPts would draw from a second stream
        mod.input_chain_for_dump(str(tmp_path), None, [0.3, 7, 1])
    flt = mod.input_chain_for_dump(str(tmp_path), None, [0.3, 7, 3])      # the golden chain + the module -> input_filters.yaml
    one, chain = facade_check(tmp_path / "one.yaml", tmp_path / "input_filters.yaml")
    assert one["error"] is None and one["modules"] == [(8, 3, 0, [F(1.0 / 3.0), F(7), F(0), F(0), F(0), F(0)])]
    assert chain["error"] is None and len(chain["modules"]) == len(flt) == 6
    for got, a in zip(chain["modules"], flt):                              # the facade's descriptor == the one the tool runs
        assert got == (a.type, a.dim, a.flag, [F(a.v[i]) for i in range(6)])
    assert chain["modules"][5][:3] == (8, 3, 1)
    # ... and the tool's run of that chain is the oracle's run of the golden chain followed by the model
    scan = _scan()
    golden = mod.input_filter_chain(os.path.join(ROOT, "tests", "golden", "input_filters.yaml"))
    front = oracle.apply_point_filters(golden, scan, seed=1)
    got = mod.run_input_filters(flt, scan, 1)
    want, leaves = M.octree_grid(front, F(0.3), 7, M.MEDOID)
    assert 1 < len(leaves) < front.shape[0] and _same(got, want)


# ---------------------------------------------------------------- GPU: through lsgpu_apply_point_filters

@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_matches_host_twin(name):
    import torch
    from laser_slam_amd import icp
    case = cases()[name]
    dev_in = torch.from_numpy(np.array(case.pts)).cuda()
    with icp.IcpHandle() as h:
        for method in METHODS:
            twin = icp.octree_grid_points(case.pts, case.max_size, case.max_point, method, SEED)
            assert twin.shape[0] == len(case.leaves)
            chain = _chain(_lib, [_spec(case.max_size, case.max_point, method)])
            got = h.apply_point_filters(chain, case.pts, seed=SEED)                            # host in, host out
            assert _same(got, twin), (name, method)
            dev = h.apply_point_filters(_chain(_lib, [_spec(case.max_size, case.max_point, method, 0)]), dev_in, seed=SEED)   # device in, device out
            assert dev.is_cuda and _same(dev.cpu().numpy(), twin), (name, method)
            if case.pts.shape[0] <= 5000:
                assert _same(got, case.want(method)), (name, method)


@pytest.mark.gpu
def test_chain_continues_the_draw_stream():
    """[OctreeGrid RandomPts, RandomSampling 0.5] with a seed == the twin followed by lsgpu_filter_random_sampling on the
    continuing stream: one draw per leaf, then one per OUTPUT point; the same chain again on the handle, unseeded, goes on
    from there."""
    from laser_slam_amd import icp
    scan = _scan()
    specs = [_spec(0.5, 7, M.RANDOM_PTS), (_lib.FILTER_RANDOM_SAMPLING, 0, 0, [0.5])]
    want = []
    for seed in (7, -1):
        a = icp.octree_grid_points(scan, 0.5, 7, M.RANDOM_PTS, seed)
        want.append(a[icp.random_sampling(a.shape[0], 0.5, -1)])
    assert 0 < want[0].shape[0] < scan.shape[0] and not _same(want[0], want[1])
    # ... which is the model with libc's draws 1 .. n_leaves, and draws n_leaves + 1 .. 2 n_leaves for RandomSampling
    n_leaves = len(cases()["scan_p7_size"].leaves)
    model, _ = M.octree_grid(scan, 0.5, 7, M.RANDOM_PTS, libc_draws(7, 0, n_leaves))
    assert _same(want[0], model[libc_draws(7, n_leaves, n_leaves) < F(0.5)])
    with icp.IcpHandle() as h:
        assert _same(h.apply_point_filters(_chain(_lib, specs), scan, seed=7), want[0])
        assert _same(h.apply_point_filters(_chain(_lib, specs), scan, seed=-1), want[1])


@pytest.mark.gpu
def test_module_anywhere_in_a_chain(oracle):
    """MaxDist in front and behind, two octree modules in one chain; one handle, clouds of changing size"""
    from laser_slam_amd import icp
    scan, small = _scan(), _scan(32, 5)
    near = [(_lib.FILTER_MAX_DIST, -1, 0, [30.0])]
    with icp.IcpHandle() as h:
        for cloud in (small, scan, small):
            a = oracle.apply_point_filters(_chain(oracle, near), cloud, seed=-1)
            b = icp.octree_grid_points(a, 0.0, 7, M.MEDOID)
            c = oracle.apply_point_filters(_chain(oracle, [(_lib.FILTER_MAX_DIST, 0, 0, [5.0])]), b, seed=-1)
            assert 0 < c.shape[0] < b.shape[0] < a.shape[0] < cloud.shape[0]
            specs = near + [_spec(0.0, 7, M.MEDOID), (_lib.FILTER_MAX_DIST, 0, 0, [5.0])]
            assert _same(h.apply_point_filters(_chain(_lib, specs), cloud), c)
            # a fine octree's centroids through a coarse one that picks at random: the second module sees the first one's output
            d = icp.octree_grid_points(cloud, 0.0, 7, M.CENTROID)
            e = icp.octree_grid_points(d, 2.0, 64, M.RANDOM_PTS, 11)
            assert 1 < e.shape[0] < d.shape[0] < cloud.shape[0]
            got = h.apply_point_filters(_chain(_lib, [_spec(0.0, 7, M.CENTROID), _spec(2.0, 64, M.RANDOM_PTS)]), cloud, seed=11)
            assert _same(got, e)


@pytest.mark.gpu
def test_device_refusals_leave_the_handle_usable():
    from laser_slam_amd import icp
    big = _uniform(np.random.default_rng(3), 500)
    dirty = big.copy()
    dirty[17, 1] = np.nan
    inf = big.copy()
    inf[3, 2] = -np.inf
    L = _lib.lib()
    case = cases()["scan_p7_size"]
    with icp.IcpHandle() as h:
        def good():
            for method in METHODS:
                want = icp.octree_grid_points(case.pts, case.max_size, case.max_point, method, SEED)
                assert _same(h.apply_point_filters(_chain(_lib, [_spec(case.max_size, case.max_point, method)]), case.pts, seed=SEED), want)
        good()
        for pts, spec, code, word in ((dirty, _spec(), _lib.BAD_ARG, "RemoveNaNDataPointsFilter"),
                                      (inf, _spec(), _lib.BAD_ARG, "RemoveNaNDataPointsFilter"),
                                      (dirty, _spec(0.5, 7, M.RANDOM_PTS), _lib.BAD_ARG, "RemoveNaNDataPointsFilter"),
                                      (big, _spec(-1.0), _lib.BAD_CONFIG, "maxSizeByNode"),
                                      (big, _spec(np.inf), _lib.BAD_CONFIG, "maxSizeByNode"),
                                      (big, _spec(np.nan), _lib.BAD_CONFIG, "maxSizeByNode"),
                                      (big, _spec(0.0, 0), _lib.BAD_CONFIG, "maxPointByNode"),
                                      (big, _spec(0.0, 1.5), _lib.BAD_CONFIG, "maxPointByNode"),
                                      (big, _spec(0.0, 2.0 ** 25), _lib.BAD_CONFIG, "maxPointByNode"),
                                      (big, _spec(0.0, 1, 4), _lib.BAD_CONFIG, "samplingMethod"),
                                      (big, _spec(0.0, 1, -1), _lib.BAD_CONFIG, "samplingMethod"),
                                      (big, _spec(0.0, 1, 0, 2), _lib.BAD_CONFIG, "buildParallel")):
            with pytest.raises(_lib.LsgpuError) as e:
                h.apply_point_filters(_chain(_lib, [spec]), pts)
            msg = L.lsgpu_last_error(h._h).decode()
            assert e.value.code == code and word in msg and "OctreeGridDataPointsFilter" in msg, spec
            good()                                                           # the next call on the handle gives the right result
        # a bad parameter anywhere in the chain is refused before anything runs: no draw is consumed
        icp.random_sampling(0, 0.5, 3)
        with pytest.raises(_lib.LsgpuError) as e:
            h.apply_point_filters(_chain(_lib, [(_lib.FILTER_RANDOM_SAMPLING, 0, 0, [0.5]), _spec(0.0, 0)]), big)
        assert e.value.code == _lib.BAD_CONFIG
        assert np.array_equal(icp.random_sampling(100, 0.5, -1), np.nonzero(libc_draws(3, 0, 100) < F(0.5))[0])
        # an emptied cloud in front of the module; the module in front of a filter that empties the cloud
        with pytest.raises(_lib.ConvergenceError):
            h.apply_point_filters(_chain(_lib, [(_lib.FILTER_MAX_DIST, -1, 0, [0.001]), _spec()]), case.pts)
        assert "no points to filter" in L.lsgpu_last_error(h._h).decode()
        good()
        with pytest.raises(_lib.ConvergenceError):
            h.apply_point_filters(_chain(_lib, [_spec()]), big[:0])
        assert h.apply_point_filters(_chain(_lib, [_spec(), (_lib.FILTER_MAX_DIST, -1, 0, [0.001])]), case.pts).shape[0] == 0
        good()
