"""Carried normals (include/lsgpu_icp.h, "carried normals"): clouds that bring their normals along -- in slots, through the
sub-map assembly, through both filter sections of a compute -- against the same work done by hand.

The yardstick is composition.  The hand-made path uses entry points that other tests pin to the oracle: lsgpu_transform_points
and lsgpu_rotate_descriptors for each member of a sub-map, concatenated; the sequential filter chain
(lsgpu_apply_point_filters, RandomSampling as a type 5 module at its place: tests/chain_cuts_cases.py) for the points a
section keeps; a numpy gather of their normals; lsgpu_orient_normals; then lsgpu_icp_set_reference +
lsgpu_icp_align_normals.  "Equal" is T_out, the iteration count, every numerical record of lsgpu_icp_get_trace and every
record of lsgpu_icp_get_normal_angle_trace, bit for bit -- and, where a section draws, the position of the library's draw
stream behind the call.

The normals of the fixtures are lsgpu_filter_surface_normal's (the host twin), knn 10, oriented towards the sensor at the
origin of the frame a scan was taken in -- what the input filter chain [SurfaceNormal, ObservationDirection, OrientNormals]
leaves.  The scans are synth.scan_pair(80): 5120 and 5104 points, cut to the sizes of each case."""
import ctypes as C
import io

import numpy as np
import pytest

from laser_slam_amd import _lib, icp, synth

import chain_cuts_cases as ccc

pytestmark = pytest.mark.gpu

SEED, PROB, ANGLE = 5, 0.5, 0.5
RS = ccc.RS
MIN_DIST = (2, -1, 0, [5.0])                          # MinDistDataPointsFilter, radial
BOX = (3, 0, 1, [-1, 1, -8, 8, -3, 3])                # BoundingBoxDataPointsFilter removeInside 1
MAX_DIST_REF = (1, -1, 0, [30.0])                     # MaxDistDataPointsFilter, radial


@pytest.fixture(scope="module")
def scans():
    """-> ref, its normals, rd, its normals, T_init; both sets of normals towards the own frame's origin"""
    ref, rd, _T_true, T_init = synth.scan_pair(80)
    rn = icp.orient_normals(ref, icp.surface_normal(ref, 10), (0, 0, 0))
    rdn = icp.orient_normals(rd, icp.surface_normal(rd, 10), (0, 0, 0))
    assert len(ref) >= 4868 and len(rd) >= 4099
    for a in (ref, rn, rd, rdn):                                  # shared by every test: read only
        a.setflags(write=False)
    return ref, rn, rd, rdn, np.asarray(T_init, np.float32)


def _handle(p2p=False, angle=None, robust=None, orient=0, sensor=(0.0, 0.0, 0.0), rd_knn=0):
    normals = None
    if angle is not None or orient or rd_knn:
        normals = dict(max_angle=-1.0 if angle is None else angle, reference_orient=orient, reference_sensor=sensor,
                       reading_sn_knn=rd_knn, reading_normals_given=0 if (angle is None or rd_knn) else 1)
    return icp.IcpHandle(None, 0, "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer", robust=robust, normals=normals)


def _digest(h, T, st):
    tr = h.trace()
    assert len(tr) == st.iterations
    na = tuple((t["rejected"], t["eps"].tobytes()) for t in h.normal_angle_trace())
    return np.ascontiguousarray(T, np.float32).tobytes(), int(st.iterations), int(st.converged), ccc.trace_bytes(h), na


def _by_hand(make, ref, rn, rd, rdn, T_init):
    """set_reference + align_normals (align without reading normals) on the sections' outputs"""
    with make() as h:
        h.set_reference(ref, rn)
        T, st = h.align_normals(rd, rdn, T_init) if rdn is not None else h.align(rd, T_init)
        return _digest(h, T, st), h.normal_angle_trace(), h.reference_normals() if rn is not None else None


def _rows(cloud):
    """point bytes -> index (the scans hold no point twice)"""
    table = {row.tobytes(): i for i, row in enumerate(np.ascontiguousarray(cloud, np.float32))}
    assert len(table) == len(cloud)
    return table


def _sequential(h, mods, cloud, normals, seed):
    """The sequential chain on `cloud` (the draw stream seeded first: seed >= 0) -> kept points, their normals, kept indices"""
    if seed >= 0:
        icp.random_sampling(0, 0.5, seed=seed)
    if not mods:
        return cloud, normals, np.arange(len(cloud))
    kept = np.ascontiguousarray(h.apply_point_filters(ccc.point_filters(mods, PROB), cloud, seed=-1))
    table = _rows(cloud)
    idx = np.array([table[row.tobytes()] for row in kept], np.int64)
    assert (np.diff(idx) > 0).all()                                      # order preserved
    return kept, (np.ascontiguousarray(normals[idx]) if normals is not None else None), idx


def _rigid(i):
    """A small rigid motion, member i's; float32 4x4"""
    a = 0.02 * (i + 1)
    c, s = np.cos(a), np.sin(a)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(a / 2), -np.sin(a / 2)], [0, np.sin(a / 2), np.cos(a / 2)]])
    T[:3, 3] = (0.1 * (i + 1), -0.05 * i, 0.02 * i)
    T = T.astype(np.float32)
    assert icp.check_rigid(T)
    return T


def _members(ref, rn, sizes, identity_at=None):
    """ref cut into members of `sizes`, each moved by the inverse of its transform (so that the sub-map is the scan again, up
    to rounding) -> [(points, normals, T or None)]; member identity_at keeps its points and gets no transform"""
    out, at = [], 0
    for i, n in enumerate(sizes):
        p, nn = ref[at:at + n], rn[at:at + n]
        at += n
        if i == identity_at:
            out.append((np.ascontiguousarray(p), np.ascontiguousarray(nn), None))
            continue
        T = _rigid(i)
        Ti = np.linalg.inv(T.astype(np.float64))
        q = p.copy()
        q[:, :3] = (p[:, :3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
        out.append((np.ascontiguousarray(q), np.ascontiguousarray((nn.astype(np.float64) @ Ti[:3, :3].T).astype(np.float32)), T))
    return out


def _submap_by_hand(h, members):
    """concat_i(T_i cloud_i) through lsgpu_transform_points / lsgpu_rotate_descriptors; an identity member as it is"""
    pts, nrm = [], []
    for p, nn, T in members:
        if len(p) == 0:
            continue
        pts.append(p if T is None else h.transform_points(T, p))
        nrm.append(None if nn is None else nn if T is None else h.rotate_descriptors(T, nn))
    have = all(x is not None for x in nrm)
    return np.ascontiguousarray(np.concatenate(pts)), (np.ascontiguousarray(np.concatenate(nrm)) if have else None)


def _upload(h, members, first_slot=1):
    slots, Ts = [], []
    for i, (p, nn, T) in enumerate(members):
        h.cloud_upload(first_slot + i, p, nn)
        assert h.cloud_has_normals(first_slot + i) == (nn is not None) and h.cloud_size(first_slot + i) == len(p)
        slots.append(first_slot + i)
        Ts.append(np.eye(4, dtype=np.float32) if T is None else T)
    return slots, Ts


def _clouds(h, members, rd, rdn, T_init, prob=-1.0, seed=SEED, **chain):
    slots, Ts = _upload(h, members)
    h.cloud_upload(0, rd, rdn)
    T, st = h.compute_clouds(0, slots, Ts, T_init, prob, chain.pop("ssn_knn", 0), 0.5, seed, **chain)
    return _digest(h, T, st)


# ------------------------------------------------------------------------------------------------ assembly

SIZES = {
    "blocks-span-members": ([1, 255, 256, 257, 0, 4099], None),   # a 256-thread block spans two and three members and an empty one
    "one": ([4868], None),
    "three": ([1000, 1500, 2368], 1),
    "table-full": ([304] * 15 + [308], 3),                        # 16 members: the table is full
    "fallback": ([286] * 16 + [292], 3),                          # 17: one launch per member
}


@pytest.mark.parametrize("name", list(SIZES))
def test_assembled_submap_is_the_members_moved_by_hand(scans, name):
    ref, rn, rd, rdn, T_init = scans
    sizes, identity_at = SIZES[name]
    assert sum(sizes) == 4868 and (name != "table-full" or len(sizes) == 16) and (name != "fallback" or len(sizes) == 17)
    rn = rn.copy()
    if identity_at is not None:                                   # a bit pattern that a multiplication by the identity would lose
        at = sum(sizes[:identity_at])
        rn[at, 2] = np.float32(-0.0) if rn[at, 2] == 0 else rn[at, 2]
        rn[at + 1] = (rn[at + 1, 0], rn[at + 1, 1], np.float32(-0.0))
    members = _members(ref[:4868], rn[:4868], sizes, identity_at)
    with _handle() as h:
        got = _clouds(h, members, rd[:2000], None, T_init)
        got_nrm = h.reference_normals()
        sub, sub_n = _submap_by_hand(h, members)
    assert len(sub) == 4868 and got_nrm.tobytes() == sub_n.tobytes()
    if identity_at is not None:
        assert np.signbit(sub_n[sum(sizes[:identity_at]) + 1, 2])
    want, _na, want_nrm = _by_hand(_handle, sub, sub_n, rd[:2000], None, T_init)
    assert got == want and want_nrm.tobytes() == got_nrm.tobytes()


def test_an_identity_member_is_copied_bit_for_bit_with_its_inf(scans):
    """An Inf coordinate in a member without a transform reaches the reference as it is: RemoveNaN keeps the point (a
    multiplication by the identity matrix would have made it NaN, and the module would have dropped it), and the grid build
    refuses the cloud -- on both paths."""
    ref, rn, rd, _rdn, T_init = scans
    members = _members(ref[:3000], rn[:3000], [1000, 1000, 1000], 1)
    with_inf = members[1][0].copy()
    with_inf[17, 0] = np.inf
    members[1] = (with_inf, members[1][1], None)
    cuts = ccc.chain_cuts([], [(6, 0, 0, [])])
    with _handle() as h:
        h.set_chain_cuts(cuts)
        with pytest.raises(_lib.LsgpuError) as e:
            _clouds(h, members, rd[:2000], None, T_init)
        assert e.value.code == _lib.BAD_ARG and "non-finite" in str(e.value)
        sub, sub_n = _submap_by_hand(h, members)
        assert np.isinf(sub[1017, 0]) and not np.isnan(sub).any()
        h.set_chain_cuts(None)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_reference(sub, sub_n)
        assert e.value.code == _lib.BAD_ARG and "non-finite" in str(e.value)


def test_one_member_without_normals_drops_them_for_the_submap(scans):
    ref, rn, rd, _rdn, T_init = scans
    members = _members(ref[:3000], rn[:3000], [1000, 1000, 1000], 1)
    members[2] = (members[2][0], None, members[2][2])
    with _handle() as h:                                          # point-to-plane: somebody reads them
        with pytest.raises(_lib.LsgpuError) as e:
            _clouds(h, members, rd[:2000], None, T_init)
        assert e.value.code == _lib.BAD_CONFIG and "slot 3" in str(e.value) and "carries no normals" in str(e.value)
    with _handle(p2p=True) as h:                                  # point-to-point: nobody does, the result is today's
        got = _clouds(h, members, rd[:2000], None, T_init)
        plain = [(p, None, T) for p, _n, T in members]
        assert _clouds(h, plain, rd[:2000], None, T_init) == got
        sub, _none = _submap_by_hand(h, plain)
    want, _na, _nrm = _by_hand(lambda: _handle(p2p=True), sub, None, rd[:2000], None, T_init)
    assert got == want


# ------------------------------------------------------------------------------------------------ sections

SECTIONS = {
    "no-reading-filter": ([], []),
    "random-sampling": ([RS], []),
    "cuts-around-sampling": ([MIN_DIST, RS, BOX], []),
    "max-dist-on-the-reference": ([RS], [MAX_DIST_REF]),
}


@pytest.mark.parametrize("nq", [255, 256, 257, 4099])
@pytest.mark.parametrize("name", list(SECTIONS))
def test_sections_keep_a_normal_with_its_point(scans, name, nq):
    ref, rn, rd, rdn, T_init = scans
    reading, reference = SECTIONS[name]
    # a reading of nq points spread over the whole scan (its first nq points are one sector: too little for an alignment)
    pick = np.linspace(0, len(rd) - 1, nq).astype(np.int64)
    rd, rdn = np.ascontiguousarray(rd[pick]), np.ascontiguousarray(rdn[pick])
    make = lambda: _handle(angle=ANGLE)
    with make() as h:
        # ---- by hand, and the conditions that make the case one
        ref_cut, rn_cut, _i = _sequential(h, reference, ref, rn, -1)
        steps = [len(_sequential(h, reading[:k], rd, rdn, SEED)[0]) for k in range(len(reading) + 1)]
        assert all(a > b for a, b in zip(steps, steps[1:])) and steps[-1] > 0, steps   # every module removes a point; RandomSampling keeps neither all nor none
        assert len(ref_cut) < len(ref) or not reference
        rd_cut, rdn_cut, _i = _sequential(h, reading, rd, rdn, SEED)
        pos_want = ccc.stream_position()
        # ---- the same chain on clouds without normals leaves the stream there too
        h.set_normals(None)
        h.set_chain_cuts(ccc.chain_cuts(reading, reference))
        prob = PROB if RS in reading else -1.0
        hp = _handle(p2p=True)
        hp.set_chain_cuts(ccc.chain_cuts(reading, reference))
        hp.compute(rd, ref, T_init, prob, 0, 0.5, SEED)
        assert ccc.stream_position() == pos_want
        hp.close()
        # ---- the new path: host pointers ...
        h.set_normals(dict(max_angle=ANGLE, reading_normals_given=1))
        T, st = h.compute(rd, ref, T_init, prob, 0, 0.5, SEED, reading_normals=rdn, reference_normals=rn)
        pos_got = ccc.stream_position()
        got = _digest(h, T, st)
        got_nrm = h.reference_normals()
        # ---- ... and slots
        got_slots = _clouds(h, [(ref, rn, None)], rd, rdn, T_init, prob)
    want, na, want_nrm = _by_hand(make, ref_cut, rn_cut, rd_cut, rdn_cut, T_init)
    assert pos_got == pos_want
    assert got_nrm.tobytes() == want_nrm.tobytes() == rn_cut.tobytes()
    assert got == want and got_slots == want
    assert len(na) == got[1]


# ------------------------------------------------------------------------------------------------ readers

def _reader_case(scans, make, with_rd_normals, orient=None):
    ref, rn, rd, rdn, T_init = scans
    with make() as h:
        rd_cut, rdn_cut, _i = _sequential(h, [RS], rd, rdn, SEED)
        T, st = h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reading_normals=rdn, reference_normals=rn)
        got, got_nrm = _digest(h, T, st), h.reference_normals()
    rn_hand = rn if orient is None else icp.orient_normals(ref, rn, orient[0], orient[1])
    want, na, want_nrm = _by_hand(make, ref, rn_hand, rd_cut, rdn_cut if with_rd_normals else None, T_init)
    assert got_nrm.tobytes() == want_nrm.tobytes() == rn_hand.tobytes()
    assert got == want
    return got, na


def test_point_to_plane_reads_the_carried_reference_normals(scans):
    got, na = _reader_case(scans, _handle, False)
    assert na == [] and got[1] > 1


def test_the_angle_filter_reads_both_sides(scans):
    ref, rn, rd, rdn, T_init = scans
    got, na = _reader_case(scans, lambda: _handle(angle=ANGLE), True)
    assert len(na) == got[1] > 1
    with _handle(angle=ANGLE) as h:                               # the hand-made path rejects some pairs, not all of them
        rd_cut, _n, _i = _sequential(h, [RS], rd, rdn, SEED)
    assert any(0 < t["rejected"] < len(rd_cut) for t in na)
    plain, _na = _reader_case(scans, _handle, False)
    assert plain != got                                           # ... and the filter matters
    # a reading that carries none: the filter is inert (rule 6), as in lsgpu_icp_align_normals(..., NULL, ...) on that handle
    with _handle(angle=ANGLE) as h:
        T, st = h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reference_normals=rn)
        inert = _digest(h, T, st)
    want, na_inert, _nrm = _by_hand(lambda: _handle(angle=ANGLE), ref, rn, rd_cut, None, T_init)
    assert inert == want and na_inert == [] and inert[:3] == plain[:3]


def test_robust_point_to_plane_distance_reads_them(scans):
    rb = dict(robust_fct="cauchy", tuning=1.0, scale_estimator="mad", distance_type="point2plane")
    got, _na = _reader_case(scans, lambda: _handle(robust=rb), False)
    rb2 = dict(rb, distance_type="point2point")
    other, _na = _reader_case(scans, lambda: _handle(robust=rb2), False)
    assert got != other


def test_the_reference_orientation_pair_runs_on_carried_normals(scans):
    ref, rn, rd, rdn, T_init = scans
    sensor = (0.5, -0.3, 0.2)
    turned = np.ascontiguousarray(-rn)                            # carried the wrong way round: the pair turns them back
    got, na = _reader_case((ref, turned, rd, rdn, T_init), lambda: _handle(angle=ANGLE, orient=1, sensor=sensor), True,
                           orient=(sensor, True))
    assert len(na) == got[1] and turned.tobytes() == (-rn).tobytes()   # (the caller's array is only read)
    import torch
    d_n = torch.from_numpy(turned).cuda()
    with _handle(angle=ANGLE, orient=1, sensor=sensor) as h:      # a device pointer of the caller's is not written either
        T, st = h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reading_normals=rdn, reference_normals=d_n)
        assert _digest(h, T, st) == got
    assert d_n.cpu().numpy().tobytes() == turned.tobytes()


def test_against_the_oracle_on_the_hand_filtered_clouds(scans, oracle):
    """tests/test_gpu_parity.py::test_align_matches_oracle_trace's assertions, on the carried path."""
    ref, rn, rd, rdn, T_init = scans
    with _handle() as h:
        rd_cut, _n, _i = _sequential(h, [RS], rd, rdn, SEED)
        Tg, stg = h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reference_normals=rn)
        trg = h.trace()
    rc, To, sto, tro = oracle.icp_compute(oracle.config_yaml(accum_double=1), rd_cut, ref, rn, synth.colmajor(T_init), 40)
    assert rc == 0
    To, Tg = synth.from_colmajor(To), Tg.astype(np.float64)
    assert stg.iterations == sto.iterations
    assert stg.converged == sto.converged
    for a, b in zip(trg, tro):  # per-iteration: same limit, same weights, same system
        assert np.float32(a["limit"]) == np.float32(b["limit"])
        assert a["n_used"] == b["n_used"]
        assert np.linalg.norm(a["A"] - b["A"]) / np.linalg.norm(b["A"]) < 1e-5
    dt, dr = synth.pose_error(To, Tg)
    assert dt <= 1e-4 and dr <= 1e-5, (dt, dr)


# ------------------------------------------------------------------------------------------------ a module wins

def test_a_normals_module_overwrites_what_the_clouds_carry(scans):
    ref, rn, rd, rdn, T_init = scans
    junk_r, junk_q = np.ascontiguousarray(rn[::-1]), np.ascontiguousarray(rdn[::-1])
    digests = []
    for nr_, nq_ in ((None, None), (junk_r, junk_q)):
        with _handle(angle=ANGLE, rd_knn=10) as h:
            digests.append(_clouds(h, [(ref, nr_, None)], rd, nq_, T_init, PROB, sn_knn=10))
            T, st = h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, sn_knn=10, reading_normals=nq_, reference_normals=nr_)
            digests.append(_digest(h, T, st))
    assert digests[0] == digests[1] == digests[2] == digests[3] and len(digests[0][4]) == digests[0][1]


def test_compute_normals_without_normals_is_compute(scans):
    ref, _rn, rd, _rdn, T_init = scans
    L = _lib.lib()
    out = []
    with icp.IcpHandle() as h:
        for fn in ("lsgpu_icp_compute", "lsgpu_icp_compute_normals"):
            ch = _lib.ChainCfg(PROB, 10, 0.5, 0, SEED)
            ti, to, st = icp._t16(T_init), np.empty(16, np.float32), _lib.IcpStats()
            q, r = np.ascontiguousarray(rd), np.ascontiguousarray(ref)
            if fn == "lsgpu_icp_compute":
                rc = L.lsgpu_icp_compute(h._h, q.ctypes.data, len(q), r.ctypes.data, len(r), icp._fp(ti), C.byref(ch), icp._fp(to), C.byref(st))
            else:
                rc = L.lsgpu_icp_compute_normals(h._h, q.ctypes.data, None, len(q), r.ctypes.data, None, len(r), icp._fp(ti), C.byref(ch),
                                                 icp._fp(to), C.byref(st))
            assert rc == _lib.OK
            out.append((to.tobytes(), st.iterations, ccc.trace_bytes(h), ccc.stream_position()))
    assert out[0] == out[1]


def test_upload_drops_and_release_frees_the_normals(scans):
    ref, rn, rd, rdn, T_init = scans
    with _handle() as h:
        h.cloud_upload(3, ref, rn)
        assert h.cloud_has_normals(3) and not h.cloud_has_normals(4)
        h.cloud_upload(3, ref)
        assert not h.cloud_has_normals(3) and h.cloud_size(3) == len(ref)
        h.cloud_upload(3, ref, rn)
        h.cloud_release(3)
        assert not h.cloud_has_normals(3) and h.cloud_size(3) == -1
        # upload + compute in one call stores the reading with its normals
        h.cloud_upload(1, ref, rn)
        T, st = h.compute_clouds_upload(0, rd, [1], None, T_init, PROB, 0, 0.5, SEED, reading_normals=rdn)
        got = _digest(h, T, st)
        assert h.cloud_has_normals(0) and h.cloud_size(0) == len(rd)
        T, st = h.compute_clouds(0, [1], None, T_init, PROB, 0, 0.5, SEED)
        assert _digest(h, T, st) == got
        T, st = h.compute_clouds_upload(0, rd, [1], None, T_init, PROB, 0, 0.5, SEED)    # the overlapped entry stores points only
        assert _digest(h, T, st) == got and not h.cloud_has_normals(0)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_by_their_texts(scans):
    ref, rn, rd, rdn, T_init = scans
    kw = dict(reading_normals=rdn, reference_normals=rn)
    # the thinning modules need the section's own normals module
    for setter, value, text in (("set_shadow", (None, 0.1), "ShadowDataPointsFilter on the reference needs the normals of a reference filter"),
                                ("set_cov_sampling", (None, (500, 1)), "CovarianceSamplingDataPointsFilter on the reference needs the normals of a reference filter")):
        with _handle() as h:
            getattr(h, setter)(value)
            with pytest.raises(_lib.LsgpuError) as e:
                h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, **kw)
            assert e.value.code == _lib.BAD_CONFIG and text in str(e.value)
    with _handle() as h:
        h.set_max_density(10.0)
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, **kw)
        assert e.value.code == _lib.BAD_CONFIG and "MaxDensityDataPointsFilter: needs the densities" in str(e.value)
    # the reading's thinning modules and its orientation pair need the reading's SurfaceNormalDataPointsFilter
    with _handle(angle=ANGLE) as h:
        for setter, value in (("set_shadow", (0.1, None)), ("set_cov_sampling", ((500, 1), None))):
            with pytest.raises(_lib.LsgpuError) as e:
                getattr(h, setter)(value)
            assert e.value.code == _lib.BAD_CONFIG and "needs the reading's SurfaceNormalDataPointsFilter" in str(e.value)
    with pytest.raises(_lib.LsgpuError) as e:
        icp.IcpHandle(normals=dict(max_angle=ANGLE, reading_normals_given=1, reading_orient=1))
    assert "needs the normals of a SurfaceNormalDataPointsFilter in front of it" in str(e.value)
    # a reference without normals that somebody reads
    with _handle() as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reading_normals=rdn)
        assert e.value.code == _lib.BAD_CONFIG and "one reference filter, ssn_knn or sn_knn in [3, 32]" in str(e.value)
    # a split-scan handle
    with _handle() as h:
        h.comm_init(0, 1, icp.comm_unique_id())
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, PROB, 0, 0.5, SEED, reference_normals=rn)
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and "carried normals" in str(e.value)


# ------------------------------------------------------------------------------------------------ the Python facade

ICP_FILE = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
            "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n"
            "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.5\n"
            "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
            "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
            "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 4\n")


def test_the_icp_file_without_a_normals_module_runs_on_carried_normals(scans):
    ref, rn, rd, rdn, T_init = scans
    o = icp.ICP()
    with pytest.raises(_lib.LsgpuError):
        o.load_from_yaml(io.StringIO(ICP_FILE))
    o.load_from_yaml(io.StringIO(ICP_FILE), carried=_lib.CARRIED_READING | _lib.CARRIED_REFERENCE)
    assert o.chain.normals.reading_normals_given == 1 and o.chain.surface_normal_knn == 0 and o.chain.reference_normal_knn == 0
    o.chain.seed = SEED
    T = o.compute(rd, ref, T_init, reading_normals=rdn, reference_normals=rn)
    got = _digest(o.handle, T, o.last_stats)
    with pytest.raises(_lib.LsgpuError) as e:                     # declared, read, and not there
        o.compute(rd, ref, T_init, reading_normals=rdn)
    assert e.value.code == _lib.BAD_CONFIG and "normals" in str(e.value)
    make = lambda: _handle(angle=ANGLE)
    with make() as h:
        rd_cut, rdn_cut, _i = _sequential(h, [RS], rd, rdn, SEED)
    want, _na, _nrm = _by_hand(make, ref, rn, rd_cut, rdn_cut, T_init)
    assert got == want


# ------------------------------------------------------------------------------------------------ the C++ facade

INPUT_CHAIN = ("- RandomSamplingDataPointsFilter:\n    prob: 0.8\n- SurfaceNormalDataPointsFilter:\n    knn: 10\n"
               "- ObservationDirectionDataPointsFilter\n- OrientNormalsDataPointsFilter\n")
TRACK_ICP_FILE = ICP_FILE.replace("      maxAngle: 0.5\n", "      maxAngle: 1.0\n")


def test_laser_track_carries_the_input_chains_normals_through_slots_and_host_submaps(tmp_path):
    """The two-file set-up end to end: LaserTrack with an input chain that ends with the normals modules and an ICP file
    without one, 8 scans of ~4 k points, sub-maps of 3.  Scans resident in slots (sub-maps assembled on the device) against
    sub-maps assembled on the host by RigidTransformation::compute + concatenate: every ICP factor bit for bit."""
    import os
    import subprocess
    import test_cpp_mirror as tcm
    exe = tcm._build(tmp_path, "track_driver.cpp", "track_driver")
    scene = synth.Scene(1234)
    n = 8
    with open(tmp_path / "poses.txt", "w") as f:
        for i in range(n):
            T = synth.se3(0.8 * i, 0.05 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(2.0 * i))
            synth.hdl64_scan(scene, T, 64, 10 + i).tofile(tmp_path / f"scan{i}.bin")
            f.write(tcm._pose_line(100000000 * i, T @ synth.se3(0.1 * i, -0.05 * i, 0, yaw=np.deg2rad(0.5 * i))))
    (tmp_path / "input_filters_normals.yaml").write_text(INPUT_CHAIN)
    (tmp_path / "icp_carried.yaml").write_text(TRACK_ICP_FILE)
    (tmp_path / "input_filters_none.yaml").write_text("")        # (what the driver reads where no chain is named)
    env = dict(os.environ, LSGPU_TEST_INPUT_FILTERS=str(tmp_path / "input_filters_normals.yaml"))
    outs = []
    for on_device in ("4", "0"):
        r = subprocess.run([exe, str(tmp_path), str(n), str(tmp_path / "icp_carried.yaml"), "3", on_device], capture_output=True,
                           text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([l for l in r.stdout.splitlines() if l.startswith(("factor ", "icp_iterations", "world_cloud "))])
    strip = lambda ls: [" ".join(l.split()[:5]) if l.startswith("icp_iterations") else l for l in ls]
    assert strip(outs[0]) == strip(outs[1])
    assert len([l for l in outs[0] if l.startswith("factor 2 ")]) == n - 1
    # without the declaration the ICP file does not load: the chain of the track's input filters makes the difference
    r = subprocess.run([exe, str(tmp_path), "1", str(tmp_path / "icp_carried.yaml"), "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "is required" in r.stdout + r.stderr
