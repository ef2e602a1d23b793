"""What lsgpu_icp_compute tells lsgpu_icp_set_reference's halves and the align it starts, what lsgpu_icp_align_normals tells
its align, and what lsgpu_icp_compute_clouds_upload tells its compute are arguments of those calls: nothing of it stays on
the handle.  These cases pin the call sequences in which something left behind would show -- a compute refused in the
middle of the reference build, after both filters, or ahead of its upload, and reading normals followed by a plain align.

All on the 4 k golden pair (pair4k): the side stream, the deferred build of the direction index (a reference of >= 1024
points around the origin) and the upload thread all run at that size.

"Equal" is the transform bit for bit, the same number of iterations, and per iteration the same trim limit (bits) and the
same number of inliers.  The cases lsgpu_icp_compute's refused guess leaves to a later lsgpu_icp_align are
tests/test_gpu_parity.py::test_a_refused_guess_leaves_nothing_behind_and_the_policy_info_reads."""
import numpy as np
import pytest

from laser_slam_amd import _lib, icp

import test_surface_normal_outlier as tsno

pytestmark = pytest.mark.gpu

SN_KNN = 10
SEED = 11


def _digest(T, st, tr):
    assert len(tr) == st.iterations
    return (np.ascontiguousarray(T, np.float32).tobytes(), st.iterations,
            [(np.float32(t["limit"]).tobytes(), int(t["n_used"])) for t in tr])


def _compute(h, rd, ref, T_init):
    """The default chain with SurfaceNormalDataPointsFilter: the reference goes to the grid build as given."""
    T, st = h.compute(rd, ref, T_init, 0.5, 0, 0.5, SEED, sn_knn=SN_KNN)
    return _digest(T, st, h.trace()), st.direction_index_launches


def _with_a_nan(ref):
    """One coordinate of one point is NaN, everything else stays."""
    dirty = ref.copy()
    at = len(ref) // 2
    dirty[at, 1] = np.nan
    bad = np.argwhere(~np.isfinite(dirty))
    assert bad.tolist() == [[at, 1]] and dirty.shape[1] == 4              # column 1 is y: a coordinate, not the homogeneous 1
    assert np.array_equal(np.delete(dirty, at, 0), np.delete(ref, at, 0))
    return dirty


def _not_rigid(T_init):
    bad = np.asarray(T_init, np.float32).copy()
    bad[:3, :3] *= 1.2
    assert abs(1.0 - np.linalg.det(bad[:3, :3].astype(np.float64))) > 1e-3 and not icp.check_rigid(bad)
    assert icp.check_rigid(np.asarray(T_init, np.float32))
    return bad


def test_a_failure_in_the_middle_of_the_reference_build_leaves_nothing_behind(pair4k):
    """(a) The NaN is found behind the grid build's host round trip: the reading's filter and the queries' order are on the
    side stream by then.  The next compute on the handle is a fresh handle's."""
    ref, rd, T_init = pair4k["ref"], pair4k["rd"], pair4k["T_init"]
    assert len(ref) >= 1024 and isinstance(rd, np.ndarray)                 # deferred index build; a host reading
    dirty = _with_a_nan(ref)
    with icp.IcpHandle() as fresh:
        want, want_launches = _compute(fresh, rd, ref, T_init)
    with icp.IcpHandle() as h:
        with pytest.raises(_lib.LsgpuError) as e:
            _compute(h, rd, dirty, T_init)
        assert e.value.code == _lib.BAD_ARG and "non-finite" in str(e.value)
        got, got_launches = _compute(h, rd, ref, T_init)
    print("direction_index_launches", got_launches, want_launches)
    assert got == want and got_launches == want_launches


def test_reading_normals_apply_to_their_align_and_to_no_other(oracle, pair4k):
    """(b) align_normals(rd, n), then align(rd) with the same device pointer and size: the second is the align of a handle
    that never saw reading normals, the first is not (maxAngle 0.5 rejects 45 % of the pairs of iteration 0:
    tests/test_surface_normal_outlier.py::test_the_angle_cases_are_not_vacuous, case plane-k1-trim)."""
    import torch
    k, p2p, _sn, ch, rb, ang, _turn, cut = tsno.CASES["plane-k1-trim"]
    rf, rn, rd, rdn, T_init = tsno._scene(oracle, pair4k, cut)
    d_rd = torch.from_numpy(rd).cuda()
    d_rdn = torch.from_numpy(np.ascontiguousarray(rdn, np.float32)).cuda()
    with tsno._handle(icp, k, p2p, ch, rb, ang) as never:
        never.set_reference(rf, rn)
        T0, st0 = never.align(d_rd, T_init)
        want = _digest(T0, st0, never.trace())
    with tsno._handle(icp, k, p2p, ch, rb, ang) as h:
        h.set_reference(rf, rn)
        T1, st1 = h.align_normals(d_rd, d_rdn, T_init)
        first = _digest(T1, st1, h.trace())
        assert [t["rejected"] > 0 for t in h.normal_angle_trace()] == [True] * st1.iterations
        ptr = d_rd.data_ptr()
        T2, st2 = h.align(d_rd, T_init)
        second = _digest(T2, st2, h.trace())
        assert d_rd.data_ptr() == ptr and h.normal_angle_trace() == []
    assert first != want
    assert second == want


def test_a_refused_guess_does_not_cancel_the_next_computes_index(pair4k):
    """(c) A guess that is not rigid is refused by the align, after both filters and the whole grid build, with the index's
    build still due.  The next compute on the handle is a fresh handle's."""
    ref, rd, T_init = pair4k["ref"], pair4k["rd"], pair4k["T_init"]
    bad = _not_rigid(T_init)
    with icp.IcpHandle() as fresh:
        want, want_launches = _compute(fresh, rd, ref, T_init)
    with icp.IcpHandle() as h:
        with pytest.raises(_lib.LsgpuError) as e:
            _compute(h, rd, ref, bad)
        assert e.value.code == _lib.BAD_ARG and "rigid" in str(e.value)
        got, got_launches = _compute(h, rd, ref, T_init)
    print("direction_index_launches", got_launches, want_launches)
    assert got == want and got_launches == want_launches


def test_the_slot_holds_the_scan_when_compute_returns_ahead_of_its_upload(pair4k):
    """(d) A reference shorter than SurfaceNormalDataPointsFilter's knn is refused before the uploader thread starts: the
    fused call stores the scan itself, and a compute from that slot is the compute from host arrays."""
    ref, rd, T_init = pair4k["ref"], pair4k["rd"], pair4k["T_init"]
    short = np.ascontiguousarray(ref[:SN_KNN - 1])
    assert 0 < len(short) < SN_KNN <= len(ref)
    with icp.IcpHandle() as h:
        want, _ = _compute(h, rd, ref, T_init)
        h.cloud_upload(0, short)
        h.cloud_upload(1, ref)
        assert h.cloud_size(0) == len(short) and h.cloud_size(2) == -1
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute_clouds_upload(2, rd, [0], None, T_init, 0.5, 0, 0.5, SEED, sn_knn=SN_KNN)
        assert e.value.code == _lib.BAD_ARG and "fewer points" in str(e.value)
        assert h.cloud_size(2) == len(rd)
        T, st = h.compute_clouds(2, [1], None, T_init, 0.5, 0, 0.5, SEED, sn_knn=SN_KNN)
        assert _digest(T, st, h.trace()) == want
