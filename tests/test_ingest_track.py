"""LaserTrackParams::ingest_on_device end to end (tests/cpp/ingest_track_check.cpp): a LaserTrack over 6 synthetic scans with
the input chain [MaxDist, RandomSampling, SurfaceNormal knn 10, ObservationDirection, OrientNormals] and an ICP file without a
normals module, 4 scans resident, sub-maps of 3 -- once through DataPointsFilters::apply and the fused upload, once through
ICP::ingestCloud, the draw stream at the same state in front of each.  The stored scans (features and normals) and the ICP
transformations are equal byte for byte; with ingest on every scan is ingested and none is uploaded."""
import subprocess

import numpy as np
import pytest

from laser_slam_amd import synth

import test_cpp_mirror as tcm

pytestmark = pytest.mark.gpu

INPUT_CHAIN = ("- MaxDistDataPointsFilter:\n    maxDist: 40\n- RandomSamplingDataPointsFilter:\n    prob: 0.8\n"
               "- SurfaceNormalDataPointsFilter:\n    knn: 10\n"
               "- ObservationDirectionDataPointsFilter\n- OrientNormalsDataPointsFilter\n")
ICP_FILE = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
            "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n"
            "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n  - SurfaceNormalOutlierFilter:\n      maxAngle: 1.0\n"
            "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
            "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
            "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n      smoothLength: 4\n")


def test_ingest_on_device_stores_the_same_scans_and_registers_the_same(tmp_path):
    exe = tcm._build(tmp_path, "ingest_track_check.cpp", "ingest_track_check")
    scene = synth.Scene(1234)
    n = 6
    with open(tmp_path / "poses.txt", "w") as f:
        for i in range(n):
            T = synth.se3(0.8 * i, 0.05 * i, synth.SENSOR_HEIGHT, yaw=np.deg2rad(2.0 * i))
            scan = synth.hdl64_scan(scene, T, 64, 10 + i)
            assert (np.linalg.norm(scan[:, :3], axis=1) > 40).any()          # MaxDist removes something
            scan.tofile(tmp_path / f"scan{i}.bin")
            f.write(tcm._pose_line(100000000 * i, T @ synth.se3(0.1 * i, -0.05 * i, 0, yaw=np.deg2rad(0.5 * i))))
    (tmp_path / "input_filters.yaml").write_text(INPUT_CHAIN)
    (tmp_path / "icp.yaml").write_text(ICP_FILE)
    r = subprocess.run([exe, str(tmp_path), str(n), "4", "3"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "ingest_track_check: ok" in r.stdout, r.stdout + r.stderr
    assert len([l for l in r.stdout.splitlines() if l.startswith("icp ")]) == n - 1
