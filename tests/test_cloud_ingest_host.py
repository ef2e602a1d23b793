"""lsgpu_cloud_ingest / lsgpu_cloud_download above and below the device: the export table, the bindings, the header's
declarations (additive: LSGPU_ABI_VERSION stays 4), and the facades -- ICP::ingestCloud, LaserTrackParams::ingest_on_device,
the shim -- compiled and run without a GPU (tests/cpp/ingest_check.cpp)."""
import ctypes as C
import os
import re
import subprocess

from laser_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
            "-I", os.path.join(ROOT, "integration")]


def test_the_two_symbols_are_exported_and_bound():
    L = _lib.lib()
    i64, fp = C.c_int64, L.lsgpu_cloud_upload_normals.argtypes[2]
    for name in ("lsgpu_cloud_ingest", "lsgpu_cloud_download"):
        assert hasattr(L, name) and name in _lib.ABI_SYMBOLS, name
    assert L.lsgpu_cloud_ingest.argtypes == [C.c_void_p, C.c_int, C.POINTER(_lib.PointFilter), C.c_int, fp, i64, i64, C.c_int, C.c_int,
                                             C.POINTER(C.c_float), fp, fp, C.POINTER(i64)]
    assert L.lsgpu_cloud_download.argtypes == [C.c_void_p, C.c_int, fp, fp, i64]
    from laser_slam_amd import icp
    assert callable(icp.IcpHandle.cloud_ingest) and callable(icp.IcpHandle.cloud_download)
    # a null handle is refused before anything is touched (no device needed to say so)
    m = i64(7)
    assert L.lsgpu_cloud_ingest(None, 0, None, 0, None, 0, -1, 0, 0, None, None, None, C.byref(m)) == _lib.BAD_ARG
    assert L.lsgpu_cloud_download(None, 0, None, None, 0) == _lib.BAD_ARG


def test_the_header_declares_them_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "lsgpu_icp.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int lsgpu_cloud_ingest(lsgpu_icp* h, int slot, lsgpu_point_filter* filters, int n_filters, const float* xyz1, int64_t n, "
            "int64_t seed, int normals_knn, int orient, const float sensor[3], float* out_xyz1, float* out_normals, int64_t* n_out);") in flat
    assert "int lsgpu_cloud_download(lsgpu_icp* h, int slot, float* out_xyz1, float* out_normals, int64_t cap_points);" in flat
    assert "#define LSGPU_ABI_VERSION 4" in hdr and _lib.lib().lsgpu_abi_version() == 4


def test_facade_shim_and_track_compile_and_default_to_the_old_path(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "ingest_check.cpp")
    exe = str(tmp_path / "ingest_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-DLSGPU_TEST_SEAMS"] + INCLUDES + [src, "-o", exe,
                          "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ingest_check: ok" in r.stdout, r.stdout + r.stderr
    # without the test seams (the shipped header), and through the GTSAM-typed overlay against the declaration-only stand-ins
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + INCLUDES + [src])
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-DINGEST_CHECK_OVERLAY", "-I", os.path.join(ROOT, "tests", "cpp", "mock"),
                        "-I", os.path.join(ROOT, "integration", "gtsam")] + INCLUDES + [src], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
