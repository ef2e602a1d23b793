"""Carried normals on the CPU: lsgpu_chain_load_carried against lsgpu_chain_load over the loader corpus, the two-file set-up
(input filters that end with the normals modules, an ICP file without one), the section plan, the input chain's tail, the
shim (tests/cpp/carried_check.cpp), and the additive ABI."""
import ctypes as C
import json
import os

import pytest

from laser_slam_amd import _lib, icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ICP_FILE = """
readingDataPointsFilters:
  - RandomSamplingDataPointsFilter:
      prob: 0.5
matcher:
  KDTreeMatcher:
    knn: 1
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.75
  - SurfaceNormalOutlierFilter:
      maxAngle: 0.5
errorMinimizer:
  PointToPlaneErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.01
      smoothLength: 4
"""


def _doc(text):
    import yaml
    d = yaml.load(text, Loader=yaml.BaseLoader)
    return d if isinstance(d, dict) else {}


@pytest.fixture(scope="module")
def corpus():
    """The documents of tests/golden/chain_loader_corpus.json (kept there as indices into a table of lines) -> [{yaml}]"""
    with open(os.path.join(ROOT, "tests", "golden", "chain_loader_corpus.json")) as f:
        raw = json.load(f)
    return [dict(yaml="".join(raw["lines"][i] for i in r["doc"])) for r in raw["entries"]]


def _carried(doc, carried):
    arr, n, _keep = icp._yaml_modules(doc)
    out = _lib.LoadedChain()
    why = C.create_string_buffer(512)
    rc = _lib.lib().lsgpu_chain_load_carried(arr, n, carried, C.byref(out), why, len(why))
    return rc, why.value.decode(), bytes(out)


def test_carried_0_is_chain_load_over_the_corpus(corpus):
    loaded = 0
    for e in corpus:
        try:
            doc = _doc(e["yaml"])
        except Exception:
            continue                                              # (not YAML: the facades refuse it before the library sees it)
        rc, why, out = icp.chain_load(doc)
        assert _carried(doc, 0) == (rc, why, bytes(out) if rc == _lib.OK else bytes(_lib.LoadedChain())), e["yaml"]
        loaded += rc == _lib.OK
        # the four part loaders under declaration 0: the bytes and texts of each
        rcp, whyp, cuts, shadow, motion, cs = icp.chain_load_parts_carried(doc, 0)
        for fn, part in ((icp.chain_load_cuts, cuts), (icp.chain_load_shadow, shadow), (icp.chain_load_motion, motion),
                         (icp.chain_load_cov_sampling, cs)):
            rc1, why1, want = fn(doc)
            assert (rc1, why1) == (rcp, whyp) and (rc1 != _lib.OK or bytes(want) == bytes(part)), (fn.__name__, e["yaml"])
    assert loaded > 20 and loaded < len(corpus)                   # both verdicts occur


def test_a_declaration_changes_no_document_that_loads_without_it(corpus):
    """What loads with carried 0 loads with every declaration, to the same bytes -- but for reading_normals_given, which a
    carried reading sets only where the chain has the angle filter and no reading module (no document of the corpus)."""
    for e in corpus:
        try:
            doc = _doc(e["yaml"])
        except Exception:
            continue
        rc, _why, out = _carried(doc, 0)
        if rc != _lib.OK:
            continue
        for carried in (1, 2, 3):
            assert _carried(doc, carried) == (rc, "", out), (carried, e["yaml"])


def test_the_two_file_set_up_needs_both_declarations():
    doc = _doc(ICP_FILE)
    required = "SamplingSurfaceNormalDataPointsFilter or SurfaceNormalDataPointsFilter is required"
    for carried, text in ((0, required), (_lib.CARRIED_READING, required),
                          (_lib.CARRIED_REFERENCE, "SurfaceNormalOutlierFilter: the reading section provides no normals")):
        rc, why, _out = _carried(doc, carried)
        assert rc == _lib.BAD_CONFIG and text in why, (carried, why)
        assert icp.chain_load_parts_carried(doc, carried)[:2] == (rc, why)
    assert icp.chain_load(doc)[:2] == _carried(doc, 0)[:2]
    rc, why, loaded = icp.chain_load(doc, _lib.CARRIED_READING | _lib.CARRIED_REFERENCE)
    assert rc == _lib.OK and why == ""
    assert loaded.normals.reading_normals_given == 1 and loaded.normals.reading_sn_knn == 0 and loaded.chain.ssn_knn == 0 and loaded.chain.sn_knn == 0
    assert _lib.lib().lsgpu_chain_load_carried(None, 0, 4, C.byref(loaded), None, 0) == _lib.BAD_ARG      # an unknown bit
    # a reading module of the file's own wins: nothing is "given"
    own = ICP_FILE.replace("      prob: 0.5\n", "      prob: 0.5\n  - SurfaceNormalDataPointsFilter:\n      knn: 7\n")
    rc, why, loaded = icp.chain_load(_doc(own), 3)
    assert rc == _lib.OK and loaded.normals.reading_normals_given == 0 and loaded.normals.reading_sn_knn == 7
    # the reference's orientation pair may stand on carried normals; the thinning modules may not, by their texts
    pair = "referenceDataPointsFilters:\n  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n"
    rc, why, loaded = icp.chain_load(_doc(pair + ICP_FILE), 3)
    assert rc == _lib.OK and loaded.normals.reference_orient == 1
    rc, why, _l = icp.chain_load(_doc(pair + ICP_FILE), _lib.CARRIED_READING)
    assert rc == _lib.BAD_CONFIG and "is implemented only as the pair" in why
    for module in ("ShadowDataPointsFilter", "CovarianceSamplingDataPointsFilter"):
        for front in ("", "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n"):
            y = "referenceDataPointsFilters:\n" + front + "  - " + module + "\n" + ICP_FILE
            rc, why, _l = icp.chain_load(_doc(y), 3)
            assert rc == _lib.BAD_CONFIG and module + " needs the normals: it may stand only behind" in why, why
    y = ICP_FILE.replace("      prob: 0.5\n", "      prob: 0.5\n  - ShadowDataPointsFilter\n")
    rc, why, _l = icp.chain_load(_doc(y), 3)
    assert rc == _lib.BAD_CONFIG and "needs the normals: it may stand only behind the reading's SurfaceNormalDataPointsFilter" in why
    y = ICP_FILE.replace("      prob: 0.5\n", "      prob: 0.5\n  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n")
    rc, why, _l = icp.chain_load(_doc(y), 3)
    assert rc == _lib.BAD_CONFIG and "is implemented only as the pair" in why


def test_python_facade_takes_the_declaration():
    import io
    o = icp.ICP()
    with pytest.raises(_lib.LsgpuError) as e:
        o.load_from_yaml(io.StringIO(ICP_FILE))
    assert "is required" in str(e.value)
    o.load_from_yaml(io.StringIO(ICP_FILE), carried=3)
    assert o.carried == 3 and o.chain.normals.reading_normals_given == 1 and o.chain.normals.max_angle == 0.5
    nc = icp.normals_cfg(o.chain.normals)
    assert _lib.lib().lsgpu_normals_config_check(C.byref(nc), 0, 1) == _lib.OK
    o.load_from_yaml(io.StringIO(ICP_FILE.replace("PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer")
                                 .replace("  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.5\n", "")))
    assert o.carried == 0 and o.chain.normals is None


def test_surface_normal_params_rule():
    L = _lib.lib()

    def check(**params):
        kv = sorted((k.encode(), str(v).encode()) for k, v in params.items())
        ps = (_lib.YamlParam * max(len(kv), 1))(*[_lib.YamlParam(k, v) for k, v in kv])
        knn, why = C.c_int(-1), C.create_string_buffer(256)
        return L.lsgpu_surface_normal_params_check(ps, len(kv), C.byref(knn), why, len(why)), knn.value, why.value.decode()
    assert check() == (_lib.OK, 5, "") and check(knn=10, keepNormals=1, epsilon=0) == (_lib.OK, 10, "")
    for params, text in ((dict(knn=2), "knn must be an integer in [3, 32]"), (dict(knn=33), "knn must be an integer in [3, 32]"),
                         (dict(keepNormals=0), "keepNormals must be 1"), (dict(epsilon=0.5), "epsilon must be 0"),
                         (dict(maxDist=3), "maxDist must be absent or inf"), (dict(ratio=1), "unknown parameter ratio")):
        rc, _knn, why = check(**params)
        assert rc == _lib.BAD_CONFIG and "SurfaceNormalDataPointsFilter" in why and text in why, (params, why)


def test_mirror_shim_and_plan(tmp_path):
    exe = str(tmp_path / "carried_check")
    import subprocess
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "cpp", "carried_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "carried_check: ok" in r.stdout, r.stdout + r.stderr


def test_laser_track_and_estimator_compile_with_the_declaration(tmp_path):
    import subprocess
    src = tmp_path / "facades.cpp"
    src.write_text('#include "laser_slam_amd/incremental_estimator.hpp"\n'
                   'int main() { laser_slam_amd::DataPointsFilters f; return f.producesNormals() ? 1 : 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), str(src)])


def test_the_abi_grew_and_changed_nothing():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "lsgpu_icp.h")).read()
    for n in ("lsgpu_cloud_upload_normals", "lsgpu_cloud_has_normals", "lsgpu_icp_compute_normals",
              "lsgpu_icp_compute_clouds_upload_normals", "lsgpu_chain_load_carried", "lsgpu_chain_load_parts_carried",
              "lsgpu_surface_normal_params_check"):
        assert hasattr(L, n) and n + "(" in hdr and n in _lib.ABI_SYMBOLS, n
    assert "#define LSGPU_ABI_VERSION 4" in hdr and L.lsgpu_abi_version() == 4
    assert "#define LSGPU_CARRIED_READING 1" in hdr and "#define LSGPU_CARRIED_REFERENCE 2" in hdr
    assert (_lib.CARRIED_READING, _lib.CARRIED_REFERENCE) == (1, 2)
    assert C.sizeof(_lib.IcpConfig) == 15 * 4 and C.sizeof(_lib.ChainCfg) == 24 and C.sizeof(_lib.NormalsCfg) == 48
    assert C.sizeof(_lib.LoadedChain) == 200
