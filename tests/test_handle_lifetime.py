"""A handle gives back what it took: device allocations, pinned allocations, events and streams are held by owning members
of lsgpu_icp, and lsgpu_dev_live_resources() counts the ones the library holds at the moment (all handles of the process).
Around a create / use / destroy cycle the count returns to where it stood, exactly."""
import ctypes as C
import gc

import pytest

from laser_slam_amd import _lib, icp


def live():
    f = _lib.lib().lsgpu_dev_live_resources
    f.restype, f.argtypes = C.c_long, []
    return int(f())


def cycle_a(p, base):
    """point-to-plane, profiled (the kNN event pool and the pay-off events exist): every stream, the slots, the loop's buffers"""
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.profile_kernels = 1
    with icp.IcpHandle(cfg) as h:
        rf, rn = icp.sampling_surface_normal(p["ref"], 10, 1.0, 0)
        h.set_reference(rf, rn)
        h.align(p["rd"], p["T_init"])                                       # (reserves the median's second select)
        h.compute(p["rd"], p["ref"], p["T_init"], reading_prob=0.5, ssn_knn=10, seed=3)   # host arrays: draw, copy and side stream
        h.cloud_upload(0, p["rd"])
        h.cloud_upload(3, p["ref"])                                         # (the vector of slots grows while slot 0 holds a cloud)
        h.compute_clouds(0, [3], None, p["T_init"], 0.5, 10, 0.5, seed=3)
        h.cloud_release(0)
        assert live() > base
    assert live() == base


def cycle_b(p, base):
    """reading normals, ShadowDataPointsFilter on both sides, a cut module per section, BoundTransformationChecker"""
    max_dist = (_lib.FILTER_MAX_DIST, -1, 0, (30.0,))
    with icp.IcpHandle(normals=dict(max_angle=0.6, reading_sn_knn=5),     # (the angle test is what reads the reading's normals)
                       shadow=(0.1, 0.1), cuts=dict(reading=(max_dist,), reference=(max_dist,)),
                       motion=dict(bound=True, max_rotation_norm=1.0, max_translation_norm=1.0)) as h:
        h.compute(p["rd"], p["ref"], p["T_init"], reading_prob=0.5, ssn_knn=10, seed=3)
        assert live() > base
    assert live() == base


@pytest.mark.gpu
def test_destroy_returns_every_resource(pair4k):
    gc.collect()
    base = live()
    cycle_a(pair4k, base)
    cycle_b(pair4k, base)
    cycle_a(pair4k, base)


@pytest.mark.gpu
def test_reading_normals_scratch_handle_is_returned(pair4k):
    with icp.IcpHandle() as h:
        before = live()
        h.reading_normals(pair4k["rd"], knn=5)          # (on a scratch handle of the call's own: it is gone on return)
        assert live() == before
