"""lsgpu_cloud_ingest (include/lsgpu_icp.h, "Ingest"): a raw scan through the input filter chain, with its normals, into a
cloud slot in one call on one handle -- against the three calls it stands for.

The yardstick is composition, as in tests/test_carried_normals.py: lsgpu_apply_point_filters, then lsgpu_icp_reading_normals on
what the point modules kept, then lsgpu_cloud_upload_normals.  "Equal" is bytewise throughout: the returned host arrays, what
lsgpu_cloud_download reads back from the slot, FixStepSampling's `state`, and the position of the library's draw stream
behind the call.  The scans are synth.scan_pair(80), 5120 and 5104 points, cut to the sizes of each case."""
import ctypes as C

import numpy as np
import pytest

from laser_slam_amd import _lib, icp, synth

import chain_cuts_cases as ccc

pytestmark = pytest.mark.gpu

SEED, PROB, ANGLE = 5, 0.5, 0.5
SENSOR = (0.5, -0.3, 0.2)                               # off the origin: the orientation depends on it
RS = ccc.RS
MAX_DIST = (1, -1, 0, [12.0])                           # MaxDistDataPointsFilter, radial
MIN_DIST = (2, -1, 0, [5.0])
FIX_STEP = (4, 0, 0, [3.0, 7.0, 1.5])                   # startStep, endStep, stepMult: the step moves 3 -> 4.5 -> 6.75
REMOVE_NAN = (6, 0, 0, [])
VOXEL = (7, 1, 1, [1.0, 1.0, 1.0])                      # useCentroid 1
OCTREE_RANDOM = (8, 1, 1, [0.0, 8.0])                   # samplingMethod 1 (RandomPts): one draw per leaf
KEEP_ALL = (1, -1, 0, [1e6])
KEEP_NONE = (1, -1, 0, [1e-3])

CHAINS = {
    "empty": [],
    "maxdist-sampling": [MAX_DIST, RS],
    "nan-mindist-fixstep-sampling": [REMOVE_NAN, MIN_DIST, FIX_STEP, RS],
    "voxel-grid": [VOXEL],
    "octree-random": [OCTREE_RANDOM],
}
NORMALS = [(0, 0)] + [(k, o) for k in (3, 10, 32) for o in (0, 1, 2)]


@pytest.fixture(scope="module")
def scans():
    ref, rd, _T_true, T_init = synth.scan_pair(80)
    assert len(ref) >= 5000 and len(rd) >= 5000
    with_nan = rd.copy()
    with_nan[[5, 100, 777], 0] = np.nan
    with_nan[2048, 2] = np.nan
    for a in (ref, rd, with_nan):                       # shared by every test: read only
        a.setflags(write=False)
    return ref, rd, with_nan, np.asarray(T_init, np.float32)


def _seed():
    icp.random_sampling(0, 0.5, seed=SEED)


def _detail(e):
    return str(e.value).split("[", 1)[1].rstrip("]")


def _b(a):
    return None if a is None else np.ascontiguousarray(a).tobytes()


def _compose(h, filters, cloud, knn, orient):
    """the three calls' first two on handle h (the stream continues) -> kept points, their normals or None"""
    kept = np.ascontiguousarray(h.apply_point_filters(filters, cloud, seed=-1)).copy()
    return kept, (h.reading_normals(kept, knn, orient, SENSOR) if knn else None)


def _slot(h, slot):
    """(point bytes, normal bytes or None, size) of a slot, read back; the size and has_normals calls agree with it"""
    p, n = h.cloud_download(slot)
    assert len(p) == h.cloud_size(slot) and (n is not None) == h.cloud_has_normals(slot)
    return _b(p), _b(n), len(p)


# ------------------------------------------------------------------------------------------------ composition

@pytest.mark.parametrize("knn,orient", NORMALS)
@pytest.mark.parametrize("name", list(CHAINS))
def test_ingest_is_the_three_calls(scans, name, knn, orient):
    ref, rd, with_nan, _T = scans
    mods = CHAINS[name]
    clouds = [with_nan if REMOVE_NAN in mods else rd, ref]          # two consecutive scans through the same chain object
    want, got = [], []
    with icp.IcpHandle() as h:
        f = ccc.point_filters(mods, PROB)
        _seed()
        for c in clouds:
            kept, nrm = _compose(h, f, c, knn, orient)
            h.cloud_upload(3, kept, nrm)
            want.append((_b(kept), _b(nrm), _slot(h, 3), [x.state for x in f]))
        want.append(ccc.stream_position())
        assert 0 < len(kept) and (not mods or len(kept) < len(ref))          # the chain removes something, not everything
    with icp.IcpHandle() as h:
        f = ccc.point_filters(mods, PROB)
        _seed()
        for c in clouds:
            pts, nrm = h.cloud_ingest(3, c, f, -1, knn, orient, SENSOR if orient else (0, 0, 0))
            assert (nrm is None) == (knn == 0)
            got.append((_b(pts), _b(nrm), _slot(h, 3), [x.state for x in f]))
        got.append(ccc.stream_position())
    assert got == want
    if FIX_STEP in mods:
        assert [s[3][2] for s in got[:2]] == [4.5, 6.75]


def test_the_normals_are_the_host_twins(scans):
    _ref, rd, _nan, _T = scans
    with icp.IcpHandle() as h:
        _seed()
        pts, nrm = h.cloud_ingest(0, rd, ccc.point_filters([MAX_DIST, RS], PROB), -1, 10, 1, SENSOR)
    want = icp.orient_normals(pts, icp.surface_normal(pts, 10), SENSOR)
    assert len(pts) > 1000 and _b(nrm) == _b(want)
    assert (np.abs(np.linalg.norm(nrm, axis=1) - 1) < 1e-3).all()
    # the pair turns some normals, not all of them, and its two settings are each other's opposite
    with icp.IcpHandle() as h:
        by_orient = []
        for orient in (0, 1, 2):
            _seed()
            by_orient.append(h.cloud_ingest(0, rd, ccc.point_filters([MAX_DIST, RS], PROB), -1, 10, orient, SENSOR)[1])
    turned = [(by_orient[o] != by_orient[0]).any(axis=1) for o in (1, 2)]
    assert _b(by_orient[1]) == _b(nrm) and 0 < turned[0].sum() < len(nrm) and 0 < turned[1].sum() < len(nrm)
    assert not (turned[0] & turned[1]).any() and (turned[0] | turned[1]).sum() >= len(nrm) - 8    # (a dot product of exactly 0 turns in neither)


def test_a_device_cloud_and_null_outputs_leave_the_same_slot(scans):
    import torch
    _ref, rd, _nan, _T = scans
    mods = [MAX_DIST, RS]
    with icp.IcpHandle() as h:
        _seed()
        pts, nrm = h.cloud_ingest(0, rd, ccc.point_filters(mods, PROB), -1, 10, 2, SENSOR)
        host = (_b(pts), _b(nrm), _slot(h, 0))
        d_rd = torch.from_numpy(np.array(rd)).cuda()
        _seed()
        d_pts, d_nrm = h.cloud_ingest(1, d_rd, ccc.point_filters(mods, PROB), -1, 10, 2, SENSOR)
        assert d_pts.is_cuda and d_nrm.is_cuda
        assert (_b(d_pts.cpu().numpy()), _b(d_nrm.cpu().numpy()), _slot(h, 1)) == host
        assert _b(d_rd.cpu().numpy()) == _b(rd)                      # the caller's device cloud is only read
        for cloud in (rd, d_rd):
            _seed()
            assert h.cloud_ingest(2, cloud, ccc.point_filters(mods, PROB), -1, 10, 2, SENSOR, download=False) == (None, None)
            assert _slot(h, 2) == host[2]
        _seed()                                                       # an empty chain on a device cloud: staged nowhere, stored all the same
        h.cloud_ingest(2, d_rd, ccc.point_filters([]), -1, 10, 2, SENSOR, download=False)
        assert _slot(h, 2)[0] == _b(rd) and _slot(h, 2)[1] == _b(h.reading_normals(rd, 10, 2, SENSOR))


# ------------------------------------------------------------------------------------------------ sizes

@pytest.mark.parametrize("chain", ["empty", "keep-all"])
@pytest.mark.parametrize("n,knn", [(255, 10), (256, 10), (257, 10), (3, 3), (513, 32)])
def test_kept_counts_around_a_block(scans, n, knn, chain):
    _ref, rd, _nan, _T = scans
    pick = np.linspace(0, len(rd) - 1, n).astype(np.int64)
    cloud = np.ascontiguousarray(rd[pick])
    mods = [] if chain == "empty" else [KEEP_ALL]
    with icp.IcpHandle() as h:
        kept, want = _compose(h, ccc.point_filters(mods), cloud, knn, 1)
        assert len(kept) == n
        h.cloud_upload(0, rd[:700])                                   # (what the slot held is gone afterwards)
        pts, nrm = h.cloud_ingest(0, cloud, ccc.point_filters(mods), -1, knn, 1, SENSOR)
        assert (_b(pts), _b(nrm)) == (_b(cloud), _b(want)) and _slot(h, 0) == (_b(cloud), _b(want), n)


def test_fewer_kept_points_than_knn_empties_the_slot(scans):
    _ref, rd, _nan, _T = scans
    two = np.ascontiguousarray(rd[[10, 2000]])
    with icp.IcpHandle() as h:
        with pytest.raises(_lib.LsgpuError) as want:
            h.reading_normals(two, 3, 0)
        assert want.value.code == _lib.BAD_ARG and "fewer points than knn" in str(want.value)
        h.cloud_upload(1, rd[:100])
        for mods, cloud in (([], two), ([KEEP_ALL], two), ([KEEP_NONE], rd[:50])):
            with pytest.raises(_lib.LsgpuError) as e:
                h.cloud_ingest(1, cloud, ccc.point_filters(mods), -1, 3, 0)
            assert e.value.code == _lib.BAD_ARG and _detail(e) == _detail(want) and h.cloud_size(1) == -1
            h.cloud_upload(1, rd[:100])
        # a NaN that reaches the normals' grid: the composition's code and text, the slot empty
        bad = np.array(rd[:64])
        bad[7, 1] = np.nan
        with pytest.raises(_lib.LsgpuError) as want:
            h.reading_normals(bad, 3, 0)
        with pytest.raises(_lib.LsgpuError) as e:
            h.cloud_ingest(1, bad, ccc.point_filters([]), -1, 3, 0)
        assert e.value.code == want.value.code == _lib.BAD_ARG and "non-finite" in _detail(e) and _detail(e) == _detail(want)
        assert h.cloud_size(1) == -1
        # ... and one that reaches VoxelGrid
        h.cloud_upload(1, rd[:100])
        with pytest.raises(_lib.LsgpuError) as want:
            h.apply_point_filters(ccc.point_filters([VOXEL]), bad)
        with pytest.raises(_lib.LsgpuError) as e:
            h.cloud_ingest(1, bad, ccc.point_filters([VOXEL]))
        assert e.value.code == want.value.code == _lib.BAD_ARG and _detail(e) == _detail(want) and h.cloud_size(1) == -1


def test_small_and_empty_clouds_without_normals(scans):
    _ref, rd, _nan, _T = scans
    with icp.IcpHandle() as h:
        one = np.ascontiguousarray(rd[77:78])
        pts, nrm = h.cloud_ingest(0, one, ccc.point_filters([KEEP_ALL]))
        assert nrm is None and _b(pts) == _b(one) and _slot(h, 0) == (_b(one), None, 1)
        # a chain whose last module keeps nothing: what apply_point_filters + an upload do
        assert len(h.apply_point_filters(ccc.point_filters([KEEP_NONE]), rd[:300])) == 0
        pts, nrm = h.cloud_ingest(0, rd[:300], ccc.point_filters([KEEP_NONE]))
        assert len(pts) == 0 and nrm is None and h.cloud_size(0) == 0 and not h.cloud_has_normals(0)
        assert _slot(h, 0) == (b"", None, 0)
        # ... and a module behind it is handed an empty cloud
        with pytest.raises(_lib.ConvergenceError) as e:
            h.cloud_ingest(0, rd[:300], ccc.point_filters([KEEP_NONE, KEEP_ALL]))
        assert "no points to filter" in str(e.value) and h.cloud_size(0) == -1
        # no points at all: a no-op for an empty chain, an error for any other
        empty = np.empty((0, 4), np.float32)
        h.cloud_upload(0, rd[:10])
        with pytest.raises(_lib.ConvergenceError) as e:
            h.cloud_ingest(0, empty, ccc.point_filters([KEEP_ALL]))
        assert e.value.code == _lib.NO_CONVERGENCE and "no points to filter" in str(e.value) and h.cloud_size(0) == -1
        pts, nrm = h.cloud_ingest(0, empty, ccc.point_filters([]))
        assert len(pts) == 0 and h.cloud_size(0) == 0


def test_the_fourth_component_travels(scans):
    _ref, rd, _nan, _T = scans
    cloud = np.array(rd)
    bits = np.random.default_rng(3).integers(0, 2 ** 32, len(cloud), dtype=np.uint64).astype(np.uint32)
    bits[:4] = (0x7FC00001, 0xFFFFFFFF, 0x80000000, 0x7F800000)     # a NaN with a payload, another, -0, +inf
    cloud.view(np.uint32)[:, 3] = bits
    for mods in ([], [MAX_DIST, RS]):
        with icp.IcpHandle() as h:
            _seed()
            kept, want = _compose(h, ccc.point_filters(mods, PROB), cloud, 10, 1)
            _seed()
            pts, nrm = h.cloud_ingest(0, cloud, ccc.point_filters(mods, PROB), -1, 10, 1, SENSOR)
            assert (_b(pts), _b(nrm)) == (_b(kept), _b(want)) and _slot(h, 0)[:2] == (_b(kept), _b(want))
            tags = pts.view(np.uint32)[:, 3]
            assert set(tags.tolist()) <= set(bits.tolist()) and (mods or (tags == bits).all())


# ------------------------------------------------------------------------------------------------ slot rules

def test_an_ingest_without_normals_drops_the_slots_normals(scans):
    _ref, rd, _nan, _T = scans
    with icp.IcpHandle() as h:
        h.cloud_ingest(0, rd, ccc.point_filters([]), -1, 10, 0, download=False)
        assert h.cloud_has_normals(0)
        info = h.info().n_reference
        assert info == len(rd)                                        # (the search ran on the handle's own grid)
        h.cloud_ingest(0, rd[:900], ccc.point_filters([]), download=False)
        assert not h.cloud_has_normals(0) and h.cloud_size(0) == 900 and _slot(h, 0) == (_b(rd[:900]), None, 900)
        assert h.info().n_reference == info                           # without normals the reference is untouched


def _raw_ingest(h, slot, filters, cloud, seed, knn, orient, sensor, out_normals=None):
    a = np.ascontiguousarray(cloud, np.float32)
    out = np.empty((max(len(a), 1), 4), np.float32)
    m = C.c_int64(-7)
    sv = None if sensor is None else icp._fp(np.asarray(sensor, np.float32))
    rc = _lib.lib().lsgpu_cloud_ingest(h._h, slot, filters, len(filters), a.ctypes.data, len(a), seed, knn, orient, sv,
                                       out.ctypes.data, None if out_normals is None else out_normals.ctypes.data, C.byref(m))
    return rc, m.value, _lib.lib().lsgpu_last_error(h._h).decode()


def test_a_configuration_error_touches_nothing(scans):
    ref, rd, _nan, _T = scans
    nrm = icp.surface_normal(ref[:500], 5)
    _seed()
    pos0 = ccc.stream_position()
    bad_prob = ccc.point_filters([MAX_DIST, RS], 1.5)
    good = ccc.point_filters([MAX_DIST, RS], PROB)
    room = np.empty((len(rd), 3), np.float32)
    cases = [("filter parameter", bad_prob, 0, 0, SENSOR, None, _lib.BAD_CONFIG, "apply_point_filters"),
             ("knn 2", good, 2, 0, SENSOR, None, _lib.BAD_ARG, "normals_knn"),
             ("knn 33", good, 33, 0, SENSOR, None, _lib.BAD_ARG, "normals_knn"),
             ("knn -1", good, -1, 0, SENSOR, None, _lib.BAD_ARG, "normals_knn"),
             ("orient 3", good, 10, 3, SENSOR, None, _lib.BAD_ARG, "orient"),
             ("orient -1", good, 10, -1, SENSOR, None, _lib.BAD_ARG, "orient"),
             ("orient without normals", good, 0, 1, SENSOR, None, _lib.BAD_ARG, "orient"),
             ("orient without sensor", good, 10, 1, None, None, _lib.BAD_ARG, "sensor"),
             ("out_normals without normals", good, 0, 0, SENSOR, room, _lib.BAD_ARG, "out_normals")]
    with icp.IcpHandle() as h:
        h.cloud_upload(2, ref[:500], nrm)
        before = _slot(h, 2)
        for what, f, knn, orient, sensor, on, code, word in cases:
            _seed()
            rc, m, why = _raw_ingest(h, 2, f, rd, 99, knn, orient, sensor, on)     # (seed 99 is not taken either)
            assert (rc, m) == (code, 0) and word in why, (what, rc, m, why)
            assert ccc.stream_position() == pos0, what
            assert _slot(h, 2) == before and before[2] == 500, what
        assert [x.state for x in good] == [0.0, 0.0]
        assert _lib.lib().lsgpu_cloud_ingest(h._h, -1, good, 2, rd.ctypes.data, len(rd), -1, 0, 0, None, None, None, None) == _lib.BAD_ARG
        # a split-scan handle is refused by name, as carried normals are there; without normals it ingests
        h.comm_init(0, 1, icp.comm_unique_id())
        rc, m, why = _raw_ingest(h, 2, good, rd, 99, 10, 0, SENSOR)
        assert rc == _lib.BAD_CONFIG and "split-scan" in why and "cloud_ingest" in why and _slot(h, 2) == before
        _seed()
        pts, _n = h.cloud_ingest(2, rd, ccc.point_filters([MAX_DIST, RS], PROB))
        assert 0 < len(pts) < len(rd) and ccc.stream_position() != pos0


def test_download_refuses_by_its_texts(scans):
    ref, _rd, _nan, _T = scans
    L = _lib.lib()
    p, q = np.empty((600, 4), np.float32), np.empty((600, 3), np.float32)
    with icp.IcpHandle() as h:
        for slot in (0, 5):                                           # never used / beyond every slot so far
            assert L.lsgpu_cloud_download(h._h, slot, p.ctypes.data, None, 600) == _lib.BAD_ARG
            assert "empty slot" in L.lsgpu_last_error(h._h).decode()
        with pytest.raises(_lib.LsgpuError) as e:
            h.cloud_download(0)
        assert e.value.code == _lib.BAD_ARG and "empty slot" in str(e.value)
        h.cloud_upload(0, ref[:500])
        assert L.lsgpu_cloud_download(h._h, 0, p.ctypes.data, None, 499) == _lib.BAD_ARG
        assert "smaller than the cloud" in L.lsgpu_last_error(h._h).decode()
        assert L.lsgpu_cloud_download(h._h, 0, p.ctypes.data, q.ctypes.data, 600) == _lib.BAD_ARG
        assert "carries no normals" in L.lsgpu_last_error(h._h).decode()
        assert L.lsgpu_cloud_download(h._h, 0, p.ctypes.data, None, 500) == _lib.OK and _b(p[:500]) == _b(ref[:500])
        h.cloud_release(0)
        assert L.lsgpu_cloud_download(h._h, 0, p.ctypes.data, None, 600) == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ through a compute

def _angle_handle():
    return icp.IcpHandle(None, 0, "PointToPlaneErrorMinimizer", normals=dict(max_angle=ANGLE, reading_normals_given=1))


def _digest(h, T, st):
    tr = h.trace()
    assert len(tr) == st.iterations
    na = tuple((t["rejected"], t["eps"].tobytes()) for t in h.normal_angle_trace())
    return np.ascontiguousarray(T, np.float32).tobytes(), int(st.iterations), int(st.converged), ccc.trace_bytes(h), na


def test_ingested_scans_register_as_uploaded_ones(scans):
    """tests/test_carried_normals.py's digest: a reading and a sub-map of three members, each ingested, against the same
    clouds placed in the slots with their normals by hand."""
    ref, rd, _nan, T_init = scans
    mods = [MAX_DIST, RS]
    raw = [rd, ref[:1700], ref[1700:3400], ref[3400:]]
    with _angle_handle() as h:
        _seed()
        kept = [_compose(h, ccc.point_filters(mods, PROB), c, 10, 1) for c in raw]
        for slot, (p, n) in enumerate(kept):
            h.cloud_upload(slot, p, n)
        T, st = h.compute_clouds(0, [1, 2, 3], None, T_init, -1.0, 0, 0.5, -1)
        want = _digest(h, T, st), ccc.stream_position()
    with _angle_handle() as h:
        _seed()
        for slot, c in enumerate(raw):
            h.cloud_ingest(slot, c, ccc.point_filters(mods, PROB), -1, 10, 1, SENSOR, download=False)
            assert h.cloud_has_normals(slot) and h.cloud_size(slot) == len(kept[slot][0])
        T, st = h.compute_clouds(0, [1, 2, 3], None, T_init, -1.0, 0, 0.5, -1)
        got = _digest(h, T, st), ccc.stream_position()
    assert got == want
    assert got[0][1] > 1 and len(got[0][4]) == got[0][1] and any(r for r, _e in got[0][4])   # the angle filter ran, and rejected


def test_set_reference_after_an_ingest_is_a_fresh_handles(scans):
    ref, rd, _nan, T_init = scans
    rf, rn = icp.sampling_surface_normal(ref, 10, 0.5, SEED)
    with icp.IcpHandle() as h:
        h.set_reference(rf, rn)
        T, st = h.align(rd[::2], T_init)
        want = _digest(h, T, st), _b(h.reference_normals())
    with icp.IcpHandle() as h:
        h.cloud_ingest(0, rd, ccc.point_filters([]), -1, 10, 1, SENSOR, download=False)
        assert h.info().n_reference == len(rd)                        # replaced, as documented
        h.set_reference(rf, rn)
        T, st = h.align(rd[::2], T_init)
        assert (_digest(h, T, st), _b(h.reference_normals())) == want
    assert want[0][1] > 1
