"""MaxDist-, MinDist-, BoundingBox- and RemoveNaNDataPointsFilter in the ICP chain's filter sections (include/lsgpu_icp.h, "cut
modules in the ICP chain"): the loader's rules through the three front ends (CPU), the fused pass of a section against the
sequential input filter chain and the CPU oracle, and lsgpu_icp_compute with the modules against compute on pre-cut clouds (GPU).
tests/chain_cuts_cases.py holds what the cases share and says how the second route is built."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

from laser_slam_amd import _lib, icp, synth

import chain_cuts_cases as cases
from chain_cuts_cases import RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL_T = 1e-4    # m     (tests/test_gpu_parity.py: compute against the oracle)
TOL_R = 1e-5    # rad

TAIL = """matcher:
  KDTreeMatcher: {knn: 1}
outlierFilters:
  - TrimmedDistOutlierFilter: {ratio: 0.75}
errorMinimizer:
  %s
transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 40}
  - DifferentialTransformationChecker: {minDiffRotErr: 0.001, minDiffTransErr: 0.01, smoothLength: 4}
"""
SSN = "  - SamplingSurfaceNormalDataPointsFilter: {knn: 10, ratio: 0.5}\n"


def document(reading="", reference=SSN, minimizer="PointToPlaneErrorMinimizer"):
    doc = ("readingDataPointsFilters:\n" + reading) if reading else ""
    doc += ("referenceDataPointsFilters:\n" + reference) if reference else ""
    return doc + TAIL % minimizer


# the document of the issue: three cut modules around RandomSampling on the reading, four in front of the sampling filter
ISSUE_DOC = document(
    "  - MinDistDataPointsFilter: {minDist: 5}\n"
    "  - RandomSamplingDataPointsFilter: {prob: 0.5}\n"
    "  - MaxDistDataPointsFilter: {maxDist: 25}\n"
    "  - BoundingBoxDataPointsFilter: {xMin: -1, xMax: 1, yMin: -8, yMax: 8, zMin: -3, zMax: 3}\n",
    "  - MaxDistDataPointsFilter: {maxDist: 30}\n"
    "  - MinDistDataPointsFilter:\n"
    "      minDist: 4.5\n"
    "      dim: -1\n"
    "  - BoundingBoxDataPointsFilter: {xMin: -40, xMax: 40, yMin: -40, yMax: 40, zMin: -2.5, zMax: 2.5, removeInside: 0}\n"
    "  - RemoveNaNDataPointsFilter\n" + SSN)

NINE = "".join("  - MaxDistDataPointsFilter: {dim: %d, maxDist: %d}\n" % (i % 3, 50 + i) for i in range(9))
NORMALS_TAIL = ("  - SurfaceNormalDataPointsFilter: {knn: 8}\n  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n")

# (document, what the refusal names)
REFUSED = [
    (document(reference=SSN + "  - MinDistDataPointsFilter: {minDist: 1}\n"),
     "referenceDataPointsFilters: MinDistDataPointsFilter behind the module that produces the normals is not implemented: the normals would have to be gathered through the cut"),
    (document(reference="  - SurfaceNormalDataPointsFilter: {knn: 8}\n  - RemoveNaNDataPointsFilter\n"),
     "referenceDataPointsFilters: RemoveNaNDataPointsFilter behind the module that produces the normals is not implemented"),
    (document(reference=SSN + "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n  - BoundingBoxDataPointsFilter\n"),
     "referenceDataPointsFilters: BoundingBoxDataPointsFilter behind the module that produces the normals is not implemented"),
    (document("  - RandomSamplingDataPointsFilter\n" + NORMALS_TAIL + "  - MaxDistDataPointsFilter\n", SSN + "  - ObservationDirectionDataPointsFilter\n  - OrientNormalsDataPointsFilter\n"),
     "readingDataPointsFilters: MaxDistDataPointsFilter behind the module that produces the normals is not implemented"),
    (document("  - SurfaceNormalDataPointsFilter: {knn: 8}\n  - MinDistDataPointsFilter\n"),
     "readingDataPointsFilters: MinDistDataPointsFilter behind the module that produces the normals is not implemented"),
    (document(NINE), "readingDataPointsFilters: MaxDistDataPointsFilter is a ninth cut module"),
    (document(reference=NINE + SSN), "referenceDataPointsFilters: MaxDistDataPointsFilter is a ninth cut module"),
    (document("  - MaxDistDataPointsFilter: {dim: 3}\n"), "MaxDistDataPointsFilter: dim must be an integer in [-1, 2]"),
    (document("  - MinDistDataPointsFilter: {dim: -2}\n"), "MinDistDataPointsFilter: dim must be an integer in [-1, 2]"),
    (document(reference="  - MinDistDataPointsFilter: {dim: 1.5}\n" + SSN), "MinDistDataPointsFilter: dim must be an integer in [-1, 2]"),
    (document("  - BoundingBoxDataPointsFilter: {removeInside: 2}\n"), "BoundingBoxDataPointsFilter: removeInside must be 0 or 1"),
    (document("  - BoundingBoxDataPointsFilter: {xMin: -1, xmax: 1}\n"), "BoundingBoxDataPointsFilter: unknown parameter xmax"),
    (document("  - RemoveNaNDataPointsFilter: {dim: 0}\n"), "RemoveNaNDataPointsFilter: unknown parameter dim"),
    (document(reference="  - MaxDistDataPointsFilter: {minDist: 3}\n" + SSN), "MaxDistDataPointsFilter: unknown parameter minDist"),
    (document("  - MaxDistDataPointsFilter: {maxDist: far}\n"), "MaxDistDataPointsFilter: maxDist is not a number"),
    (document(reference="  - BoundingBoxDataPointsFilter: {zMax: 2m}\n" + SSN), "BoundingBoxDataPointsFilter: zMax is not a number"),
    (document("  - MinDistDataPointsFilter: {minDist: .nan}\n"), "MinDistDataPointsFilter: minDist is not a number"),
    # what stays refused as it was
    (document("  - FixStepSamplingDataPointsFilter: {startStep: 2}\n"), "readingDataPointsFilters: module FixStepSamplingDataPointsFilter is not implemented on the HIP path"),
    (document(reference="  - FixStepSamplingDataPointsFilter\n" + SSN), "referenceDataPointsFilters: module FixStepSamplingDataPointsFilter is not implemented on the HIP path"),
    (document("  - VoxelGridDataPointsFilter\n"), "readingDataPointsFilters: module VoxelGridDataPointsFilter is not implemented on the HIP path"),
    (document(reference="  - MaxDistDataPointsFilter\n  - VoxelGridDataPointsFilter: {vSizeX: 1}\n" + SSN), "referenceDataPointsFilters: module VoxelGridDataPointsFilter is not implemented on the HIP path"),
    (document("  - MinDistDataPointsFilter\n  - SurfaceNormalDataPointsFilter: {knn: 8}\n  - RandomSamplingDataPointsFilter\n"),
     "SurfaceNormalDataPointsFilter before RandomSamplingDataPointsFilter"),
    (document(reference="  - MaxDistDataPointsFilter\n" + SSN + "  - SurfaceNormalDataPointsFilter: {knn: 8}\n"), "referenceDataPointsFilters: one module at most"),
    (document("  - MinDistDataPointsFilter\n  - RandomSamplingDataPointsFilter\n  - MaxDistDataPointsFilter\n  - RandomSamplingDataPointsFilter\n"),
     "RandomSamplingDataPointsFilter given twice"),
]

# documents with cut modules that load: (document, cut modules of the reading with RS in its place, of the reference)
F32 = lambda v: tuple(float(str(np.float32(x))) for x in v)   # (the shortest decimal of the float32: what the document said)
INF = float("inf")
ACCEPTED = [
    (ISSUE_DOC, cases.READING, cases.REFERENCE),
    # point-to-point: cut modules alone in the reference section; no reading section at all
    (document(reference="  - RemoveNaNDataPointsFilter\n  - MaxDistDataPointsFilter: {dim: 2, maxDist: .5}\n", minimizer="PointToPointErrorMinimizer"),
     [], [(6, 0, 0, []), (1, 2, 0, [0.5])]),
    # defaults; no RandomSampling; inf where the input chain's parser takes it; a module given three times
    (document("  - MaxDistDataPointsFilter\n  - MinDistDataPointsFilter\n  - BoundingBoxDataPointsFilter\n  - MaxDistDataPointsFilter: {maxDist: inf}\n"
              "  - MaxDistDataPointsFilter: {maxDist: -.inf, dim: 0}\n"),
     [(1, -1, 0, [1.0]), (2, -1, 0, [1.0]), (3, 0, 1, [-1, 1, -1, 1, -1, 1]), (1, -1, 0, [INF]), (1, 0, 0, [-INF])], []),
    # RandomSampling last, the reading's normals behind the cuts, SurfaceNormal as the reference filter behind eight
    (document("  - BoundingBoxDataPointsFilter: {xMin: -.inf, removeInside: 1}\n  - RandomSamplingDataPointsFilter: {prob: 0.25}\n" + NORMALS_TAIL,
              "".join("  - MinDistDataPointsFilter: {dim: %d, minDist: 0.%d}\n" % (i % 3, i + 1) for i in range(8)) + "  - SurfaceNormalDataPointsFilter: {knn: 8}\n")
     .replace("outlierFilters:\n", "outlierFilters:\n  - SurfaceNormalOutlierFilter: {maxAngle: 1.0}\n"),
     [(3, 0, 1, [-INF, 1, -1, 1, -1, 1]), RS], [(2, i % 3, 0, [(i + 1) / 10.0]) for i in range(8)]),
]


def expected_cuts(reading, reference):
    c = cases.chain_cuts(reading, reference)
    pad = lambda ms: tuple((t, d, f, F32(tuple(v) + (0.0,) * (6 - len(v)))) for t, d, f, v in ms)
    return icp.ChainCuts(pad(c.reading), pad(c.reference), c.reading_sampling_at)


def python_load(text):
    """The Python front end on a document -> (rc, why, LoadedChain, ChainCuts struct or None, ICP.chain or the error raised)"""
    doc = yaml.load(text, Loader=yaml.BaseLoader) or {}
    rc, why, lc = icp.chain_load(doc)
    rc2, why2, cc = icp.chain_load_cuts(doc)
    assert (rc2, why2) == (rc, why)                         # one rule set: the same verdict and the same text
    o = icp.ICP()
    try:
        o.load_from_yaml(io.StringIO(text))
        got = o.chain
    except _lib.LsgpuError as err:
        got = err
    return rc, why, lc, cc, got


@pytest.fixture(scope="module")
def cpp_lines(tmp_path_factory):
    """tests/cpp/cut_loader_check.cpp (the C++ facade) over every document of this file: {document: its line}"""
    docs = [d for d, _ in REFUSED] + [d for d, _, _ in ACCEPTED]
    docs += [open(os.path.join(ROOT, "tests", "golden", n)).read() for n in ("icp_chain.yaml", "icp_chain_tight.yaml")]
    tmp = tmp_path_factory.mktemp("chain_cuts")
    exe, path = str(tmp / "cut_loader_check"), str(tmp / "docs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "cut_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    with open(path, "wb") as f:
        for d in docs:
            b = d.encode()
            f.write(b"DOC %d\n" % len(b) + b)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "cut_loader_check: ok %d" % len(docs), r.stdout[-2000:] + r.stderr
    return dict(zip(docs, lines[:-1]))


def test_a_document_with_cut_modules_loads(cpp_lines):
    """The issue's document (refused before the cut modules existed: "module MinDistDataPointsFilter is not implemented on the
    HIP path") and three more: the values, the order and reading_sampling_at, the same bytes from all three front ends."""
    for text, reading, reference in ACCEPTED:
        rc, why, lc, cc, chain = python_load(text)
        assert rc == _lib.OK and why == "" and isinstance(chain, icp.ChainConfig), (text, why, chain)
        want = expected_cuts(reading, reference)
        assert icp._chain_cuts(cc) == want and chain.cuts == want, (text, icp._chain_cuts(cc), want)
        assert list(lc.reserved)[2:] == [len(want.reading), len(want.reference), 0, 0] and cc.reserved == 0
        assert chain == icp._chain_config(lc, cc) and chain != icp._chain_config(lc)
        assert chain.reading_sampling_prob == (-1.0 if RS not in reading else 0.5 if text is ISSUE_DOC else 0.25)
        kind, a, b = cpp_lines[text].split(" ")
        assert kind == "OK" and bytes.fromhex(a) == bytes(lc) and bytes.fromhex(b) == bytes(cc), cpp_lines[text]
    rc, why, lc, cc, chain = python_load(ISSUE_DOC)
    assert (cc.n_reading, cc.n_reference, cc.reading_sampling_at) == (3, 4, 1)
    assert [f.type for f in cc.reading[:3]] == [2, 1, 3] and [f.type for f in cc.reference[:4]] == [1, 2, 3, 6]
    assert cc.reading[0].v[0] == 5.0 and cc.reading[1].v[0] == 25.0 and list(cc.reading[2].v) == [-1, 1, -8, 8, -3, 3] and cc.reading[2].flag == 1
    assert cc.reference[1].v[0] == 4.5 and cc.reference[2].flag == 0 and bytes(cc.reading[3]) == bytes(48) and bytes(cc.reference[4]) == bytes(48)
    assert (lc.chain.reading_prob, lc.chain.ssn_knn, lc.chain.ssn_ratio, lc.icp.trim_ratio) == (0.5, 10, 0.5, 0.75)


def test_refusals_name_the_module(cpp_lines):
    for text, names in REFUSED:
        rc, why, lc, cc, raised = python_load(text)
        assert rc == _lib.BAD_CONFIG and names in why, (text, why)
        assert isinstance(raised, _lib.LsgpuError) and raised.code == _lib.BAD_CONFIG and why in str(raised), (text, raised)
        assert cpp_lines[text] == "ERR " + why, (cpp_lines[text], why)


def test_chains_without_cut_modules_load_to_the_bytes_they_did(cpp_lines):
    with open(os.path.join(ROOT, "tests", "golden", "chain_cuts_parent_chains.json")) as f:
        recorded = json.load(f)["chains"]
    assert sorted(recorded) == ["icp_chain.yaml", "icp_chain_tight.yaml"]
    for name, hx in recorded.items():
        text = open(os.path.join(ROOT, "tests", "golden", name)).read()
        rc, why, lc, cc, chain = python_load(text)
        assert rc == _lib.OK and bytes(lc) == bytes.fromhex(hx) and len(bytes(lc)) == 200 and list(lc.reserved) == [0] * 6
        assert bytes(cc) == bytes(C.sizeof(_lib.ChainCuts)) and chain.cuts is None and "cuts" not in chain.extra
        assert chain == icp._chain_config(lc)
        assert cpp_lines[text] == "OK " + hx + " -"
    assert icp.ChainConfig() == icp.ChainConfig(extra={}) and icp.ChainConfig().cuts is None


def test_struct_layout_and_conversions():
    assert C.sizeof(_lib.PointFilter) == 48 and C.sizeof(_lib.ChainCuts) == 16 + 2 * 8 * 48 and _lib.CHAIN_CUT_MAX == 8
    assert C.sizeof(_lib.LoadedChain) == 200
    want = expected_cuts(cases.READING, cases.REFERENCE)
    cc = icp.chain_cuts_cfg(want)
    assert icp._chain_cuts(cc) == want and icp.chain_cuts_cfg(cc) is cc
    assert bytes(icp.chain_cuts_cfg(dict(reading=want.reading, reference=want.reference, reading_sampling_at=1))) == bytes(cc)
    for s in ("lsgpu_icp_set_chain_cuts", "lsgpu_icp_filter_section", "lsgpu_chain_load_cuts"):
        assert s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s)


def test_the_loader_alone(tmp_path):
    """tests/cpp/cut_loader_check.cpp built with -DCUT_LOADER_STANDALONE against csrc/lsgpu_chain_loader.cpp alone: both entry
    points on module lists built in C++ (the build a sanitizer run of the loader uses)."""
    exe = str(tmp_path / "cut_loader_standalone")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-DCUT_LOADER_STANDALONE", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cut_loader_check.cpp"),
                           os.path.join(ROOT, "laser_slam_amd", "csrc", "lsgpu_chain_loader.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("cut_loader_check (standalone): ok"), r.stdout[-2000:] + r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU

BOX = [-1, 1, -8, 8, -3, 3]
SECTION_LISTS = {
    "max_radial": [(1, -1, 0, [25.0])], "max_x": [(1, 0, 0, [3.0])], "max_y": [(1, 1, 0, [-2.0])], "max_z": [(1, 2, 0, [0.25])],
    "min_radial": [(2, -1, 0, [5.0])], "min_x": [(2, 0, 0, [3.0])], "min_y": [(2, 1, 0, [2.0])], "min_z": [(2, 2, 0, [0.5])],
    "box_inside": [(3, 0, 0, [-30, 30, -8, 8, -3, 3])], "box_outside": [(3, 0, 1, BOX)], "remove_nan": [(6, 0, 0, [])],
    "eight": [(6, 0, 0, []), (1, -1, 0, [40.0]), (2, -1, 0, [3.0]), (3, 0, 1, BOX), (1, 2, 0, [1.5]), (2, 1, 0, [0.05]), (3, 0, 0, [-35, 35, -35, 35, -3, 3]),
              (1, 0, 0, [30.0])],
    "sampling_first": [RS, (2, -1, 0, [5.0]), (1, -1, 0, [25.0])],
    "sampling_middle": [(2, -1, 0, [5.0]), RS, (1, -1, 0, [25.0]), (3, 0, 1, BOX)],
    "sampling_last": [(2, -1, 0, [5.0]), (3, 0, 1, BOX), RS],
    "sampling_alone": [RS],
    "keeps_everything": [(3, 0, 1, [100, 101, 100, 101, 100, 101]), (3, 0, 1, [-101, -100, 0, 1, 0, 1])],   # (a NaN is not inside a box)
    "keeps_everything_sampled": [(3, 0, 1, [100, 101, 100, 101, 100, 101]), RS],
    "keeps_nothing": [(6, 0, 0, []), (1, -1, 0, [0.0])],
    "keeps_nothing_sampled": [RS, (2, -1, 0, [5.0]), (1, -1, 0, [0.0])],
}
# wave and block edges, a partial last block, more than one scan element -- at most 17 block counts: one launch and one sub-tile
# of the scan; the multi-tile scan of the block counts (from 1 048 577 points on) is covered in tests/test_primitive_sizes.py
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def pair():
    ref, rd, T_true, T_init = synth.scan_pair(64)
    assert (len(ref), len(rd)) == (4096, 4080)
    return dict(ref=ref, rd=rd, T_init=T_init)


@pytest.fixture(scope="module")
def handle():
    with icp.IcpHandle() as h:
        yield h


def section_cloud(pair, n):
    """The first n points of the pair's reading (4099: with the reference's first 19 behind it), a NaN planted in x, in z and in
    the pad of three points (fewer points: they share)"""
    p = np.concatenate([pair["rd"], pair["ref"][:19]])[:n].copy()
    assert len(p) == n
    p[0, 0] = np.nan
    p[min(n - 1, 37), 2] = np.nan
    p[n - 1, 3] = np.nan
    return p


def sequential(h, oracle, mods, p, seed):
    """lsgpu_apply_point_filters and the oracle's input chain on p -> (points, the library's stream position).  A module that
    is handed an empty cloud ends both with an error: the chain has left no point."""
    try:
        out = np.ascontiguousarray(h.apply_point_filters(cases.point_filters(mods), p, seed=seed))
    except _lib.ConvergenceError:
        out = np.empty((0, 4), np.float32)
    pos = cases.stream_position()
    ora = oracle.apply_point_filters(cases.point_filters(mods, cls=oracle.PointFilter), p, seed=seed)
    assert np.array_equal(out, np.empty((0, 4), np.float32) if ora is None else ora, equal_nan=True)
    return out, pos


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SECTION_LISTS))
def test_filter_section_equals_the_sequential_chain(name, pair, handle, oracle):
    mods = SECTION_LISTS[name]
    cuts = cases.chain_cuts(mods)
    for n in SIZES:
        p = section_cloud(pair, n)
        want, want_pos = sequential(handle, oracle, mods, p, 5)
        got = handle.filter_section(cuts, 0, p, prob=cases.PROB if RS in mods else -1.0, seed=5)
        pos = cases.stream_position()
        assert got.tobytes() == want.tobytes() and pos == want_pos, (name, n, len(got), len(want))
        if "everything" in name and RS not in mods:
            assert len(got) == n
        if "nothing" in name:
            assert len(got) == 0
        if RS not in mods:                                   # the reference's side of the same modules
            ref_side = handle.filter_section(icp.ChainCuts((), cuts.reading, 0), 1, p, prob=0.5, seed=5)
            assert ref_side.tobytes() == want.tobytes() and cases.stream_position() == want_pos
    if name in ("eight", "sampling_middle"):                 # enough is cut, and enough is left, for the comparison to mean something
        assert 0.05 * SIZES[-1] < len(got) < 0.9 * SIZES[-1], len(got)


@pytest.mark.gpu
def test_filter_section_on_device_pointers(pair, handle):
    import torch
    mods = SECTION_LISTS["sampling_middle"]
    p = section_cloud(pair, 4099)
    want = np.ascontiguousarray(handle.apply_point_filters(cases.point_filters(mods), p, seed=5))
    want_pos = cases.stream_position()
    d = torch.from_numpy(p).cuda()
    got = handle.filter_section(cases.chain_cuts(mods), 0, d, prob=cases.PROB, seed=5)
    assert got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes() and cases.stream_position() == want_pos
    assert d.cpu().numpy().tobytes() == p.tobytes()           # the input is only read


def both_routes(make_handle, reading, reference, pair, **chain):
    a = cases.route_a(make_handle, reading, reference, pair["rd"], pair["ref"], pair["T_init"], **chain)
    b = cases.route_b(make_handle, reading, reference, pair["rd"], pair["ref"], pair["T_init"], **chain)
    assert a[1] >= 3, a[1]
    assert a[0] == b[0], (np.frombuffer(a[0], np.float32), np.frombuffer(b[0], np.float32))      # T_out
    assert a[1] == b[1] and a[2] == b[2] and len(a[2]) > 0                                      # iterations, trace
    assert a[3] == b[3]                                                                         # the draw stream
    assert a[4] == b[4]
    return a, b


@pytest.mark.gpu
def test_compute_with_cuts_equals_compute_on_cut_clouds(pair):
    """The issue's case 2.  The cuts alone keep 2999 of 4080 reading points and 3634 of 4096 reference points (the CPU oracle
    says so too); each section keeps between 50 % and 95 %."""
    a, b = both_routes(icp.IcpHandle, cases.READING, cases.REFERENCE, pair)
    with icp.IcpHandle() as h:
        cut_rd = h.apply_point_filters(cases.point_filters([m for m in cases.READING if m != RS]), pair["rd"])
        cut_ref = h.apply_point_filters(cases.point_filters(cases.REFERENCE), pair["ref"])
        assert (len(cut_rd), len(cut_ref)) == (2999, 3634)
        assert len(h.apply_point_filters(cases.point_filters(cases.REFERENCE[:2]), pair["ref"])) == 3634   # the last two remove nothing
    for kept, n in ((len(cut_rd), 4080), (len(cut_ref), 4096), (b[5][1], 4096)):
        assert 0.5 * n <= kept <= 0.95 * n
    assert 0.2 * 4080 < b[5][0] < 0.5 * 4080                  # ... and RandomSampling halves what reaches it
    # every cut module in front of RandomSampling: the module is left to compute on the pre-cut reading
    front = [m for m in cases.READING if m != RS] + [RS]
    a2, b2 = both_routes(icp.IcpHandle, front, cases.REFERENCE, pair)
    assert b2[5] == (2999, 3634) and a2[0] != a[0]            # (another chain: other draws for other points)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["surface_normal_reference", "point_to_point", "reading_normals", "robust", "covariance", "matcher_knn_3"])
def test_compute_with_cuts_on_other_chains(case, pair):
    chain, reading, reference = {}, cases.READING, cases.REFERENCE
    kw = {}
    if case == "surface_normal_reference":
        chain = dict(ssn_knn=0, sn_knn=8)
    elif case == "point_to_point":
        kw, chain = dict(error_minimizer="PointToPointErrorMinimizer"), dict(ssn_knn=0)
    elif case == "reading_normals":
        kw = dict(normals=icp.NormalsConfig(1.0, 8, 1, 1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    elif case == "robust":
        kw = dict(robust=icp.RobustConfig("huber", 1.5, "mad", 0, "point2point", float("inf")))
    elif case == "covariance":
        kw = dict(covariance=0.01)
    elif case == "matcher_knn_3":
        kw = dict(matcher_knn=3)
    handles = []

    def make():
        handles.append(icp.IcpHandle(**kw))
        return handles[-1]
    if case == "covariance":                                  # the quality record is read while the handle lives
        quality = []
        orig = make

        class Keep:
            def __init__(self):
                self.h = orig()

            def __enter__(self):
                return self.h.__enter__()

            def __exit__(self, *a):
                quality.append(self.h.quality())
                return self.h.__exit__(*a)
        both_routes(Keep, reading, reference, pair, **chain)
        qa, qb = quality
        assert qa["covariance"].tobytes() == qb["covariance"].tobytes() and qa["n_pairs"] == qb["n_pairs"] and qa["residual"] == qb["residual"]
        assert np.all(np.isfinite(qa["covariance"])) and qa["n_pairs"] > 100
    else:
        both_routes(make, reading, reference, pair, **chain)


@pytest.mark.gpu
def test_compute_clouds_with_cuts(pair):
    """A two-slot sub-map with a sub-map transform that is not the identity: the cut modules see the ASSEMBLED sub-map; the
    slots hold afterwards what was uploaded.  compute_clouds_upload: the same result, the same draws."""
    ref, rd, T_init = pair["ref"], pair["rd"], pair["T_init"]
    T1 = synth.se3(0.4, -0.2, 0.05, yaw=np.deg2rad(3.0)).astype(np.float32)
    half = len(ref) // 2
    with icp.IcpHandle() as h:
        part1 = np.ascontiguousarray(h.transform_points(np.linalg.inv(T1.astype(np.float64)).astype(np.float32), ref[half:]))
        submap = np.concatenate([ref[:half], np.ascontiguousarray(h.transform_points(T1, part1))])
    results = []
    for upload in (False, True):
        with icp.IcpHandle() as h:
            h.set_chain_cuts(cases.chain_cuts(cases.READING, cases.REFERENCE))
            h.cloud_upload(1, ref[:half]); h.cloud_upload(2, part1)
            if upload:
                T, st = h.compute_clouds_upload(0, rd, [1, 2], [np.eye(4, dtype=np.float32), T1], T_init, cases.PROB, seed=cases.SEED)
            else:
                h.cloud_upload(0, rd)
                T, st = h.compute_clouds(0, [1, 2], [np.eye(4, dtype=np.float32), T1], T_init, cases.PROB, seed=cases.SEED)
            results.append((T.tobytes(), int(st.iterations), cases.trace_bytes(h), cases.stream_position()))
            # the slots hold what was uploaded: a second call gives the same, and without the cut modules the slots give ...
            for slot, cloud in ((0, rd), (1, ref[:half]), (2, part1)):
                assert h.cloud_size(slot) == len(cloud)
            Tb, stb = h.compute_clouds(0, [1, 2], [np.eye(4, dtype=np.float32), T1], T_init, cases.PROB, seed=cases.SEED)
            assert Tb.tobytes() == T.tobytes() and stb.iterations == st.iterations
            h.set_chain_cuts(None)
            Tn, stn = h.compute_clouds(0, [1, 2], [np.eye(4, dtype=np.float32), T1], T_init, cases.PROB, seed=cases.SEED)
        with icp.IcpHandle() as h:                            # ... what a handle that never had any gives for the raw clouds
            Tf, stf = h.compute(rd, submap, T_init, cases.PROB, seed=cases.SEED)
        assert Tn.tobytes() == Tf.tobytes() and stn.iterations == stf.iterations
    b = cases.route_b(icp.IcpHandle, cases.READING, cases.REFERENCE, rd, submap, T_init)
    for r in results:
        assert r == (b[0], b[1], b[2], b[3])
    assert 0.5 * 4096 <= b[5][1] <= 0.95 * 4096


@pytest.mark.gpu
def test_compute_with_cuts_without_the_side_stream(pair):
    """LSGPU_NO_SIDE_STREAM=1 (read once per process: a fresh child): the reading's section behind the grid build on the main
    stream.  Both routes in the child agree, and agree with this process, where the section runs on the side stream."""
    env = dict(os.environ, LSGPU_NO_SIDE_STREAM="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "chain_cuts_cases.py")], env=env, capture_output=True, text=True, timeout=120)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CUTS_RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(line[0][len("CUTS_RESULT "):])
    assert res["a"] == res["b"]
    a = cases.route_a(icp.IcpHandle, cases.READING, cases.REFERENCE, pair["rd"], pair["ref"], pair["T_init"])
    assert res["iterations"] == a[1] and np.array(res["T"], np.float32).tobytes() == a[0]


@pytest.mark.gpu
def test_compute_with_cuts_against_the_oracle(pair, oracle):
    """The CPU oracle end to end on case 2: its input chain on both clouds (RandomSampling at its place in the reading's, behind
    the reference filter's draws), then its ICP -- iterations, every iteration's limit and inlier count, T within 1e-4 m /
    1e-5 rad.  And its whole ICP::compute on the clouds cut with every module in front of RandomSampling."""
    ref, rd, T_init = pair["ref"], pair["rd"], pair["T_init"]
    of = lambda mods: cases.point_filters(mods, cls=oracle.PointFilter)
    cut_ref = oracle.apply_point_filters(of(cases.REFERENCE), ref)
    rf, rn = oracle.sampling_surface_normal(cut_ref, 10, 0.5, cases.SEED)
    cut_rd = oracle.apply_point_filters(of(cases.READING), rd, seed=-1)
    rc, To, sto, tro = oracle.icp_compute(oracle.config_yaml(accum_double=1), cut_rd, rf, rn, synth.colmajor(T_init), 40)
    assert rc == 0
    with icp.IcpHandle() as h:
        h.set_chain_cuts(cases.chain_cuts(cases.READING, cases.REFERENCE))
        T, st = h.compute(rd, ref, T_init, cases.PROB, seed=cases.SEED)
        tr = h.trace()
        assert h.info().n_reference == len(rf)
        assert st.iterations == sto.iterations == len(tr) and st.final_n_used == sto.final_n_used
        for t, o in zip(tr, tro):
            assert np.float32(t["limit"]) == np.float32(o["limit"]) and t["n_used"] == o["n_used"]
        dt, dr = synth.pose_error(T, synth.from_colmajor(To))
        assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
        # every cut module in front: oracle.apply_point_filters, then oracle.icp_compute_full (0 after 7 iterations)
        front = [m for m in cases.READING if m != RS]
        pre_rd = oracle.apply_point_filters(of(front), rd)
        assert (len(pre_rd), len(cut_ref)) == (2999, 3634)
        rc, To, sto = oracle.icp_compute_full(oracle.config_yaml(accum_double=1), pre_rd, cut_ref, synth.colmajor(T_init), seed=cases.SEED)
        assert rc == 0 and sto.iterations == 7
        h.set_chain_cuts(cases.chain_cuts(front + [RS], cases.REFERENCE))
        T, st = h.compute(rd, ref, T_init, cases.PROB, seed=cases.SEED)
        assert st.iterations == sto.iterations and st.final_n_used == sto.final_n_used
        assert st.final_limit == sto.final_limit or abs(st.final_limit - sto.final_limit) < 1e-6 * sto.final_limit
        dt, dr = synth.pose_error(T, synth.from_colmajor(To))
        assert dt <= TOL_T and dr <= TOL_R, (dt, dr)


def default_result(h, pair):
    T, st = h.compute(pair["rd"], pair["ref"], pair["T_init"], cases.PROB, seed=cases.SEED)
    return T.tobytes(), int(st.iterations), cases.trace_bytes(h), cases.stream_position()


@pytest.mark.gpu
def test_errors_leave_the_handle_usable(pair):
    ref, rd, T_init = pair["ref"], pair["rd"], pair["T_init"]
    with icp.IcpHandle() as h:
        fresh = default_result(h, pair)
    nothing = (1, -1, 0, (0.0,))
    with icp.IcpHandle() as h:
        def fails(cuts, code, text, **chain):
            h.set_chain_cuts(cuts)
            with pytest.raises(_lib.LsgpuError) as e:
                h.compute(rd, ref, T_init, cases.PROB, seed=cases.SEED, **chain)
            assert e.value.code == code and text in str(e.value), str(e.value)
            assert isinstance(e.value, _lib.ConvergenceError) == (code == _lib.NO_CONVERGENCE)
            h.set_chain_cuts(None)
            assert default_result(h, pair) == fresh
        fails(icp.ChainCuts((nothing,), (), 1), _lib.NO_CONVERGENCE, "the reading filter left no point")
        fails(icp.ChainCuts(((2, -1, 0, (5.0,)), nothing), (), 1), _lib.NO_CONVERGENCE, "the reading filter left no point")
        fails(icp.ChainCuts((), ((6, 0, 0, ()), nothing), 0), _lib.NO_CONVERGENCE, "the reference filter left no point")
        # 5 reference points survive: fewer than SurfaceNormalDataPointsFilter's knn
        radii = np.sort(np.sqrt((ref[:, :3].astype(np.float64) ** 2).sum(1)))
        assert radii[5] - radii[4] > 1e-3
        r5 = float(0.5 * (radii[4] + radii[5]))
        few = icp.ChainCuts((), ((1, -1, 0, (r5,)),), 0)
        assert len(h.filter_section(few, 1, ref)) == 5
        fails(few, _lib.BAD_ARG, "fewer points than SurfaceNormalDataPointsFilter's knn", ssn_knn=0, sn_knn=8)
        # bad structs: the module named, the handle keeps what it had
        good = cases.chain_cuts(cases.READING, cases.REFERENCE)
        h.set_chain_cuts(good)
        with_cuts = default_result(h, pair)
        assert with_cuts != fresh
        bad = []
        for t in (0, 4, 5, 7, -1):
            bad.append((icp.ChainCuts(((t, 0, 0, ()),), (), 0), "type %d" % t))
        bad.append((icp.ChainCuts(((1, 3, 0, (1.0,)),), (), 0), "MaxDistDataPointsFilter: dim"))
        bad.append((icp.ChainCuts((), ((2, -2, 0, (1.0,)),), 0), "MinDistDataPointsFilter: dim"))
        nine = _lib.ChainCuts()
        nine.n_reading = 9
        bad.append((nine, "readingDataPointsFilters: 0 to 8 cut modules (MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter), not 9"))
        neg = _lib.ChainCuts()
        neg.n_reference = -1
        bad.append((neg, "referenceDataPointsFilters: 0 to 8 cut modules"))
        for cuts, text in bad:
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_chain_cuts(cuts)
            assert e.value.code == _lib.BAD_CONFIG and text in str(e.value), str(e.value)
            with pytest.raises(_lib.LsgpuError) as e:
                h.filter_section(cuts, 0, rd)
            assert e.value.code == _lib.BAD_CONFIG and text in str(e.value), str(e.value)
        assert default_result(h, pair) == with_cuts
        # switching them off: what a fresh handle computes (NULL, and a struct with no module)
        h.set_chain_cuts(icp.ChainCuts())
        assert h.cuts is None and default_result(h, pair) == fresh
        h.set_chain_cuts(good)
        h.set_chain_cuts(None)
        assert default_result(h, pair) == fresh


@pytest.mark.gpu
def test_the_split_scan_mode_refuses_cut_modules(pair):
    good = cases.chain_cuts(cases.READING, cases.REFERENCE)
    uid = icp.comm_unique_id()
    with icp.IcpHandle() as h:
        fresh = default_result(h, pair)
        h.set_chain_cuts(good)
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, uid)
        assert e.value.code == _lib.BAD_CONFIG and "MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter" in str(e.value)
        h.set_chain_cuts(None)
        assert default_result(h, pair) == fresh
    with icp.IcpHandle() as h:
        h.comm_init(0, 1, uid)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_chain_cuts(good)
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and "MaxDist" in str(e.value)
        assert h.cuts is None


@pytest.mark.gpu
def test_the_python_facade_runs_the_loaded_document(pair):
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(ISSUE_DOC))
    o.chain.seed = cases.SEED
    T = o.compute(pair["rd"], pair["ref"], pair["T_init"])
    a = cases.route_a(icp.IcpHandle, cases.READING, cases.REFERENCE, pair["rd"], pair["ref"], pair["T_init"])
    assert T.tobytes() == a[0] and o.last_stats.iterations == a[1] and bytes(o.handle.cuts) == bytes(icp.chain_cuts_cfg(o.chain.cuts))
