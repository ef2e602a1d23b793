"""ShadowDataPointsFilter behind the normals of either filter section: the host twin against an independent float32
restatement, the loader through both front ends, the ABI's layout and symbols (CPU); the device pass against the host twin and
ICP.compute with the module against the same compute assembled by hand, bit for bit (GPU).

The contract is in include/lsgpu_icp.h ("ShadowDataPointsFilter"): value = |n / |n| . p / |p||, in float with one rounding per
operation and sums left to right; a point is kept iff value > eps.  Everything below compares bits: there is no tolerance."""
import ctypes as C
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import yaml

from laser_slam_amd import _lib, icp, synth
import shadow_cases as cases
from shadow_cases import PAIR_RD, PAIR_REF, RS, SN, SN_DENS, SN_RD, SNO, SSN, TRIM, chain, shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ CPU: the host twin

def np_shadow(p, n, eps):
    """The module restated with numpy float32 arrays: every elementwise operation rounds once, sums go left to right."""
    p, n = np.asarray(p, F), np.asarray(n, F)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        lp = np.sqrt((px * px + py * py) + pz * pz)
        ux, uy, uz = nx / ln, ny / ln, nz / ln
        vx, vy, vz = px / lp, py / lp, pz / lp
        value = np.abs((ux * vx + uy * vy) + uz * vz)
        assert value.dtype == F
        keep = value > F(eps)
    return p[keep], n[keep], value


SPECIAL = [   # (point, normal, kept at eps 0.1?)
    ((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), False),                   # a zero normal
    ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), False),                   # a point at the origin
    ((1.0, 2.0, 3.0), (0.0, np.nan, 1.0), False),                # a NaN normal component
    ((1.0, np.nan, 3.0), (0.0, 0.0, 1.0), False),                # a NaN coordinate
    ((0.0, 0.0, 2.0), (0.0, 0.0, 7.0), True),                    # an unnormalised normal of length 7: value 1
    ((3.0, 4.0, 0.0), (1.0, 0.0, 0.0), True),                    # the tie row: value float32(0.6)
]


def special_cloud(n=1000, seed=3):
    """~1000 points with random unit-ish normals, the special rows spread among them -> (points, normals, rows of the specials)"""
    rng = np.random.default_rng(seed)
    p = np.ones((n, 4), F)
    p[:, :3] = rng.uniform(-20, 20, (n, 3))
    p[:, 3] = rng.uniform(0, 2, n)                               # the 4th component is not read: anything
    v = rng.normal(size=(n, 3))
    v = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.9, 1.1, (n, 1))).astype(F)
    rows = np.linspace(5, n - 1, len(SPECIAL)).astype(int)      # (the last row of the cloud is one of them)
    for r, (pt, nr, _k) in zip(rows, SPECIAL):
        p[r, :3] = pt
        v[r] = nr
    return p, v, rows


def test_host_twin_equals_the_float32_restatement():
    p, v, rows = special_cloud()
    tie = F(0.6)
    below = np.nextafter(tie, F(0))
    assert np_shadow(p[rows[5]:rows[5] + 1], v[rows[5]:rows[5] + 1], 0.1)[2].view(np.uint32)[0] == tie.view(np.uint32)
    for eps in (0.1, 0.0, float(tie), float(below), 0.5, 0.999):
        want_p, want_n, value = np_shadow(p, v, eps)
        got_p, got_n = icp.shadow(p, v, eps)
        assert len(got_p) == len(got_n) == len(want_p), (eps, len(got_p), len(want_p))       # n_out
        assert np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_n), bits(want_n)), eps   # the survivors, in order
        if eps in (0.1, 0.5):
            assert 0.05 * len(p) < len(got_p) < 0.95 * len(p)
    # the special rows at eps 0.1; the tie row is dropped at eps == its value and kept at the float just below
    kept = {tuple(r) for r in bits(icp.shadow(p, v, 0.1)[0]).tolist()}
    for r, (_pt, _nr, k) in zip(rows, SPECIAL):
        assert (tuple(bits(p[r]).tolist()) in kept) == k, r
    tp, tn = p[rows[5]:rows[5] + 1], v[rows[5]:rows[5] + 1]
    with pytest.raises(_lib.ConvergenceError):
        icp.shadow(tp, tn, float(tie))
    assert len(icp.shadow(tp, tn, float(below))[0]) == 1
    # refused: an eps out of range, outputs that are the inputs
    for bad in (-0.5, 3.2, float("nan"), float("inf")):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.shadow(p, v, bad)
        assert e.value.code == _lib.BAD_CONFIG
    k = C.c_int64(7)
    assert _lib.lib().lsgpu_filter_shadow(p.ctypes.data, v.ctypes.data, len(p), 0.1, p.ctypes.data, v.ctypes.data, C.byref(k)) == _lib.BAD_ARG
    assert k.value == 0


# ------------------------------------------------------------------------------------------------ CPU: the loader

COV = "PointToPlaneWithCovErrorMinimizer"
# documents that load -> (reading eps, reference eps)
ACCEPTED = [
    # the module on both sides, in front of the orientation pair ...
    (chain(reading=RS + SN_RD + shadow("0.2") + PAIR_RD, reference=SSN + shadow("0.3") + PAIR_REF, outliers=TRIM + SNO), (0.2, 0.3)),
    # ... behind it ...
    (chain(reading=RS + SN_RD + PAIR_RD + shadow("0.2"), reference=SN + PAIR_REF + shadow("0.3"), outliers=TRIM + SNO), (0.2, 0.3)),
    # ... behind MaxDensityDataPointsFilter
    (chain(reading=RS + SN_RD + shadow("0.25"), reference=SN_DENS + cases.max_density("50") + shadow("3.1416") + PAIR_REF, outliers=TRIM + SNO), (0.25, 3.1416)),
    (chain(reference=SN_DENS + cases.max_density("50") + PAIR_REF + shadow("0")), (None, 0.0)),
    # the default eps; the reference alone; a point-to-point chain (the normals are computed for the module)
    (chain(reference=SSN + "  - ShadowDataPointsFilter\n"), (None, 0.1)),
    (chain(reference=SN + shadow("1e-1"), minimizer="PointToPointErrorMinimizer"), (None, 0.1)),
]
# (document, words the refusal must hold)
REFUSALS = [
    # in front of the normals module
    (chain(reference=shadow() + SSN), ("ShadowDataPointsFilter", "needs the normals")),
    (chain(reading=RS + shadow() + SN_RD, outliers=TRIM + SNO), ("ShadowDataPointsFilter", "needs the normals")),
    (chain(reading=shadow() + RS), ("ShadowDataPointsFilter", "needs the normals")),
    # a chain with no reference normals module
    (chain(reference=shadow(), minimizer="PointToPointErrorMinimizer"), ("ShadowDataPointsFilter", "needs the normals")),
    # inside the orientation pair
    (chain(reference=SSN + PAIR_REF.replace("  - OrientNormals", shadow() + "  - OrientNormals")), ("ShadowDataPointsFilter", "between")),
    (chain(reading=RS + SN_RD + "  - ObservationDirectionDataPointsFilter\n" + shadow() + "  - OrientNormalsDataPointsFilter\n", outliers=TRIM + SNO),
     ("ShadowDataPointsFilter", "between")),
    # eps out of range, not a number, not finite; an unknown parameter
    (chain(reference=SSN + shadow("-0.1")), ("ShadowDataPointsFilter", "eps")),
    (chain(reference=SSN + shadow("3.2")), ("ShadowDataPointsFilter", "eps")),
    (chain(reference=SSN + shadow("abc")), ("ShadowDataPointsFilter", "eps")),
    (chain(reference=SSN + shadow(".inf")), ("ShadowDataPointsFilter", "eps")),
    (chain(reference=SSN + shadow() + "      bogus: 1\n"), ("ShadowDataPointsFilter", "bogus")),
    # a second instance
    (chain(reference=SSN + shadow() + shadow()), ("ShadowDataPointsFilter", "twice")),
    (chain(reading=RS + SN_RD + shadow() + shadow(), outliers=TRIM + SNO), ("ShadowDataPointsFilter", "twice")),
    # together with the covariance minimizer
    (chain(reference=SSN + shadow(), minimizer=COV), (COV, "ShadowDataPointsFilter")),
    # on the reading of a chain without SurfaceNormalOutlierFilter
    (chain(reading=RS + SN_RD + shadow()), ("ShadowDataPointsFilter", "SurfaceNormalOutlierFilter")),
    # in front of MaxDensityDataPointsFilter: the densities' rule stays as it is
    (chain(reference=SN_DENS + shadow() + cases.max_density("50")), ("keepDensities 1",)),
]


def _load(text):
    doc = yaml.load(text, Loader=yaml.BaseLoader) or {}
    return icp.chain_load(doc), icp.chain_load_cuts(doc), icp.chain_load_shadow(doc)


@pytest.fixture(scope="module")
def corpus_docs():
    with open(os.path.join(ROOT, "tests", "golden", "chain_loader_corpus.json")) as f:
        raw = json.load(f)
    return ["".join(raw["lines"][i] for i in r["doc"]) for r in raw["entries"]]


@pytest.fixture(scope="module")
def cpp_lines(corpus_docs, tmp_path_factory):
    """tests/cpp/shadow_loader_check.cpp over ACCEPTED, REFUSALS and the loader corpus -> (its lines, its LAYOUT line)"""
    tmp = tmp_path_factory.mktemp("shadow_loader")
    exe, docs = str(tmp / "shadow_loader_check"), str(tmp / "docs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "shadow_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    texts = [d for d, _ in ACCEPTED] + [d for d, _ in REFUSALS] + corpus_docs
    with open(docs, "wb") as f:
        for t in texts:
            b = t.encode()
            f.write(b"DOC %d\n" % len(b) + b)
    r = subprocess.run([exe, docs], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "shadow_loader_check: ok %d" % len(texts), r.stdout[-2000:] + r.stderr
    assert lines[-2].startswith("LAYOUT ")
    return lines[:-2], lines[-2]


def _eps_word(e):
    return "-" if e is None else "%.9g" % float(F(e))


def test_documents_with_the_module_load_through_both_facades(cpp_lines):
    """The test that fails without the feature: on the commit before, both facades refuse every one of these documents with
    "referenceDataPointsFilters: module ShadowDataPointsFilter is not implemented on the HIP path" (or readingDataPointsFilters)."""
    for (text, (rd_eps, ref_eps)), line in zip(ACCEPTED, cpp_lines[0]):
        (rc, why, lc), (rc2, why2, cc), (rc3, why3, sc) = _load(text)
        assert rc == rc2 == rc3 == _lib.OK, (text, why, why2, why3)
        for got, want in ((sc.reading_eps, rd_eps), (sc.reference_eps, ref_eps)):
            assert (got == -1.0) if want is None else (F(got) == F(want)), (text, got, want)
        assert tuple(sc.reserved) == (0, 0)
        o = icp.ICP()
        o.load_from_yaml(io.StringIO(text))
        assert o.chain.shadow == (None if rd_eps is None else float(str(F(rd_eps))), None if ref_eps is None else float(str(F(ref_eps))))
        # the C++ facade: the same eps, the same bytes of the two structs
        assert line == "OK %s %s %s %s" % (_eps_word(rd_eps), _eps_word(ref_eps), bytes(lc).hex(), bytes(cc).hex()), text
    # the document without the module next to one with it: the same lsgpu_loaded_chain
    with_m, without = ACCEPTED[0][0], ACCEPTED[0][0].replace(shadow("0.2"), "").replace(shadow("0.3"), "")
    assert bytes(_load(with_m)[0][2]) == bytes(_load(without)[0][2])
    assert icp.ICP().chain.shadow is None


def test_refusals_name_the_module_through_both_facades(cpp_lines):
    lines = cpp_lines[0][len(ACCEPTED):len(ACCEPTED) + len(REFUSALS)]
    for (text, words), line in zip(REFUSALS, lines):
        (rc, why, _lc), (rc2, why2, _cc), (rc3, why3, _sc) = _load(text)
        assert rc == rc2 == rc3 == _lib.BAD_CONFIG and why == why2 == why3, (text, why, why2, why3)
        for w in words:
            assert w in why, (text, why)
        with pytest.raises(_lib.LsgpuError) as e:
            icp.ICP().load_from_yaml(io.StringIO(text))
        assert e.value.code == _lib.BAD_CONFIG and why in str(e.value)
        assert line == "ERR " + why, (text, line)


def test_documents_without_the_module_load_to_the_parents_bytes(corpus_docs, cpp_lines):
    """tests/golden/shadow_parent_loader_bytes.json: lsgpu_loaded_chain and lsgpu_chain_cuts of every document of the loader
    corpus (and the text of every refusal), recorded with the library of the commit before the module loaded."""
    with open(os.path.join(ROOT, "tests", "golden", "shadow_parent_loader_bytes.json")) as f:
        parent = json.load(f)["entries"]
    lines = cpp_lines[0][len(ACCEPTED) + len(REFUSALS):]
    assert len(parent) == len(corpus_docs) == len(lines) > 300
    assert sum(e[0] == "OK" for e in parent) > 100 and sum(e[0] == "ERR" for e in parent) > 100
    zero_cuts = bytes(C.sizeof(_lib.ChainCuts)).hex()
    for text, rec, line in zip(corpus_docs, parent, lines):
        (rc, why, lc), (rc2, why2, cc), (rc3, why3, sc) = _load(text)
        if rec[0] == "OK":
            assert rc == rc2 == rc3 == _lib.OK, (text, why)
            assert bytes(lc).hex() == rec[1] and bytes(cc).hex() == (rec[2] or zero_cuts), text
            assert sc.reading_eps == -1.0 and sc.reference_eps == -1.0
            assert line == "OK - - %s %s" % (rec[1], rec[2] or zero_cuts), text
        else:
            assert rc == rc2 == rc3 == _lib.BAD_CONFIG and why == why2 == why3 == rec[1], (text, why, rec[1])
            assert line == "ERR " + rec[1], text


# ------------------------------------------------------------------------------------------------ CPU: the ABI

def test_struct_layout_symbols_and_abi_version(cpp_lines):
    L = _lib.lib()
    S = _lib.ShadowCfg
    layout = [int(x) for x in cpp_lines[1].split()[1:]]
    assert layout == [C.sizeof(S), S.reading_eps.offset, S.reference_eps.offset, S.reserved.offset] == [16, 0, 4, 8]
    assert L.lsgpu_abi_version() == 4
    with open(os.path.join(ROOT, "include", "lsgpu_icp.h")) as f:
        header = f.read()
    assert "#define LSGPU_ABI_VERSION 4\n" in header
    names = set(re.findall(r"\b(lsgpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))   # every function the header names
    new = {"lsgpu_shadow_config_default", "lsgpu_shadow_config_check", "lsgpu_shadow_config_why", "lsgpu_icp_set_shadow",
           "lsgpu_icp_filter_shadow", "lsgpu_filter_shadow", "lsgpu_chain_load_shadow"}
    assert new <= names and len(names) > 80
    for name in sorted(names):
        assert hasattr(L, name), name
    assert new <= set(_lib.ABI_SYMBOLS)
    # the default and the check / why pair
    c = S()
    c.reading_eps = c.reference_eps = 5.0
    c.reserved[0] = 9
    L.lsgpu_shadow_config_default(C.byref(c))
    assert (c.reading_eps, c.reference_eps, tuple(c.reserved)) == (-1.0, -1.0, (0, 0))
    assert L.lsgpu_shadow_config_check(C.byref(c)) == _lib.OK and L.lsgpu_shadow_config_why(C.byref(c)) is None
    for rd, ref, ok in ((0.0, -1.0, True), (-1.0, 3.1416, True), (0.1, 0.1, True), (3.2, -1.0, False), (-1.0, float("nan"), False),
                        (float("inf"), 0.1, False), (float("nan"), -1.0, False)):
        c.reading_eps, c.reference_eps = rd, ref
        assert (L.lsgpu_shadow_config_check(C.byref(c)) == _lib.OK) == ok, (rd, ref)
        why = L.lsgpu_shadow_config_why(C.byref(c))
        assert (why is None) == ok and (ok or b"ShadowDataPointsFilter" in why)
    c.reading_eps, c.reference_eps = 0.1, 0.1
    c.reserved[1] = 1
    assert L.lsgpu_shadow_config_check(C.byref(c)) == _lib.BAD_CONFIG
    assert L.lsgpu_shadow_config_check(None) == _lib.BAD_CONFIG


# ------------------------------------------------------------------------------------------------ GPU: the pass

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 4099)


def pattern_cloud(n, pattern, seed=0):
    """n points off the origin; a kept point's normal lies along its ray (value 1 up to rounding), a dropped point's across
    it (value 0 up to rounding): eps 0.1 separates them whatever the rounding"""
    rng = np.random.default_rng(seed * 7919 + n)
    p = np.ones((n, 4), F)
    p[:, :3] = rng.uniform(1, 20, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    keep = {"all": np.ones(n, bool), "last": np.arange(n) == n - 1, "half": rng.random(n) < 0.5, "none": np.zeros(n, bool)}[pattern]
    along = p[:, :3].astype(np.float64)
    across = np.cross(along, rng.normal(size=(n, 3)))
    v = np.where(keep[:, None], along, across)
    v = (v / np.linalg.norm(v, axis=1)[:, None] * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    return p, v, keep


@pytest.fixture(scope="module")
def handle():
    with icp.IcpHandle() as h:
        yield h


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_device_pass_equals_the_host_twin(n, handle):
    """Wave and block edges, a partial last block, more than one scan element (at most 17 block counts: one launch, one
    sub-tile of the scan -- the multi-tile scan of the block counts, from 1 048 577 points on, is covered in
    tests/test_primitive_sizes.py); all kept, only the last point kept, about half kept, nothing kept; host pointers and
    device pointers."""
    import torch
    for pattern in ("all", "last", "half", "none"):
        p, v, keep = pattern_cloud(n, pattern)
        if pattern == "none":
            for args in ((p, v), (torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda())):
                with pytest.raises(_lib.ConvergenceError) as e:
                    handle.filter_shadow(*args, 0.1)
                assert "left no point" in str(e.value)
            continue
        want_p, want_n = icp.shadow(p, v, 0.1)
        assert len(want_p) == keep.sum() and np.array_equal(bits(want_p), bits(p[keep])), (n, pattern)
        got_p, got_n = handle.filter_shadow(p, v, 0.1)
        assert len(got_p) == len(want_p), (n, pattern, len(got_p), len(want_p))
        assert np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_n), bits(want_n)), (n, pattern)
        dp, dv = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
        got_p, got_n = handle.filter_shadow(dp, dv, 0.1)
        assert got_p.is_cuda and got_n.is_cuda and len(got_p) == len(want_p)
        assert np.array_equal(bits(got_p.cpu().numpy()), bits(want_p)) and np.array_equal(bits(got_n.cpu().numpy()), bits(want_n)), (n, pattern)
        assert np.array_equal(bits(dp.cpu().numpy()), bits(p)) and np.array_equal(bits(dv.cpu().numpy()), bits(v))   # the inputs are only read


@pytest.mark.gpu
def test_device_pass_on_the_special_rows(handle):
    p, v, rows = special_cloud()
    tie = F(0.6)
    for eps in (0.1, 0.0, float(tie), float(np.nextafter(tie, F(0))), 0.5):
        want_p, want_n = icp.shadow(p, v, eps)
        got_p, got_n = handle.filter_shadow(p, v, eps)
        assert len(got_p) == len(want_p) and np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_n), bits(want_n)), eps
    for bad in (-0.5, 3.2, float("nan")):
        with pytest.raises(_lib.LsgpuError) as e:
            handle.filter_shadow(p, v, bad)
        assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value)
    k = C.c_int64(0)
    rc = _lib.lib().lsgpu_icp_filter_shadow(handle._h, p.ctypes.data, v.ctypes.data, len(p), 0.1, p.ctypes.data, v.ctypes.data, C.byref(k))
    assert rc == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ GPU: compute

@pytest.fixture(scope="module")
def pair():
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    assert (len(ref), len(rd)) == (4096, 4080)
    return dict(ref=ref, rd=rd, T_init=T_init)


_ROUTE_A = {}


def route_a(name, pair):
    """computed once per case, shared by the tests that need it"""
    if name not in _ROUTE_A:
        _ROUTE_A[name] = cases.route_a(cases.cases()[name], pair["rd"], pair["ref"], pair["T_init"])
    return _ROUTE_A[name]


KNN = {"reference": 10, "reading": 7}
SIDES = {"sampling": ("reference",), "surface_normal": ("reference",), "max_density": ("reference",), "point_to_point": ("reference",),
         "reading": ("reading",), "both": ("reference", "reading")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIDES))
def test_compute_with_the_module_equals_the_compute_by_hand(name, pair):
    """Route a: the loaded document through the Python facade, end to end.  Route b: the kernel-level entries, the module's
    HOST twin, set_reference + align_normals.  T_out, the stats' result fields, the whole trace, the reference the handle
    holds and the draw stream: equal."""
    a, pos_a = route_a(name, pair)
    b, pos_b, counts = cases.route_b(cases.cases()[name], pair["rd"], pair["ref"], pair["T_init"])
    print(name, "handed to the module / kept:", counts, "iterations", a[1])
    assert tuple(sorted(counts)) == tuple(sorted(SIDES[name]))
    for side, (n_in, kept) in counts.items():                   # a module that drops nothing shows nothing
        assert kept < n_in and kept >= KNN[side], (name, side, n_in, kept)
    assert a[1] >= 3 and len(a[5]) > 0
    assert a[0] == b[0], (np.frombuffer(a[0], F), np.frombuffer(b[0], F))                           # T_out
    assert a[1:5] == b[1:5]                                                                       # iterations, converged, final limit, final n_used
    assert a[5] == b[5]                                                                           # the trace
    assert a[6] == b[6] and ("reference" not in counts or a[6] == counts["reference"][1])         # the reference the handle holds
    assert pos_a == pos_b                                                                         # the draw stream


@pytest.mark.gpu
def test_compute_without_the_side_stream(pair):
    """LSGPU_NO_SIDE_STREAM=1 (read once per process: a fresh child): the chains whose reading runs on the side stream, both
    routes in the child, against route a of this process."""
    env = dict(os.environ, LSGPU_NO_SIDE_STREAM="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shadow_cases.py")], env=env, capture_output=True, text=True, timeout=120)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("SHADOW_RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(line[0][len("SHADOW_RESULT "):])
    assert set(res) == set(cases.SIDE_CASES)
    for name in cases.SIDE_CASES:
        assert res[name]["a"] == res[name]["b"] == cases.digest(*route_a(name, pair)), name


def _default_result(h, pair):
    T, st = h.compute(pair["rd"], pair["ref"], pair["T_init"], 0.5, 10, 0.5, 11)
    return T.tobytes(), int(st.iterations), int(st.final_n_used), cases.trace_bytes(h)


@pytest.mark.gpu
def test_an_emptied_section_is_an_error_that_leaves_the_handle_usable(pair):
    rd, ref, T_init = pair["rd"], pair["ref"], pair["T_init"]
    with icp.IcpHandle() as h:
        fresh = _default_result(h, pair)
    # value <= 1 < 3.1416: everything is dropped
    with icp.IcpHandle(shadow=(None, 3.1416)) as h:
        for kw in (dict(ssn_knn=10), dict(ssn_knn=0, sn_knn=10)):
            with pytest.raises(_lib.ConvergenceError) as e:
                h.compute(rd, ref, T_init, 0.5, seed=11, **kw)
            assert "the reference filter left no point" in str(e.value)
        h.set_shadow(None)
        assert h.shadow is None and _default_result(h, pair) == fresh
    nc = icp.NormalsConfig(0.6, 7, 1, 1)
    with icp.IcpHandle(normals=nc, shadow=(3.1416, None)) as h:
        with pytest.raises(_lib.ConvergenceError) as e:
            h.compute(rd, ref, T_init, 0.5, 10, 0.5, 11)
        assert "the reading filter left no point" in str(e.value)
        h.set_shadow(None)
        h.set_normals(None)
        assert _default_result(h, pair) == fresh
    # the module on a chain with no reference normals: refused by name
    with icp.IcpHandle(error_minimizer="PointToPointErrorMinimizer", shadow=(None, 0.1)) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, 0.5, 0, 0.5, 11)
        assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value)


@pytest.mark.gpu
def test_refusals_on_the_handle_in_either_order():
    """A GPU test because lsgpu_icp_create opens the device: without one there is no handle to refuse anything."""
    uid = icp.comm_unique_id()
    both = ("PointToPlaneWithCovErrorMinimizer", "ShadowDataPointsFilter")
    with icp.IcpHandle() as h:
        h.set_shadow((None, 0.1))
        assert h.shadow == (-1.0, float(F(0.1)))
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_covariance(0.01)
        assert e.value.code == _lib.BAD_CONFIG and all(w in str(e.value) for w in both)
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, uid)
        assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value)
        for bad in ((None, 3.2), (float("nan"), 0.1), (None, float("inf"))):     # a bad value: the handle keeps what it had
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_shadow(bad)
            assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value)
        assert h.shadow == (-1.0, float(F(0.1))) and h.covariance is None
        # the reading's module without the reading's normals
        for normals in (None, icp.NormalsConfig(0.6, reading_normals_given=1)):
            h.set_normals(normals)
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_shadow((0.1, None))
            assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value) and "SurfaceNormalDataPointsFilter" in str(e.value)
        # ... and the other order: the normals may not leave while the reading's module is on
        h.set_normals(icp.NormalsConfig(0.6, 7, 0, 0))
        h.set_shadow((0.1, None))
        for normals in (None, icp.NormalsConfig(0.6, reading_normals_given=1)):
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_normals(normals)
            assert e.value.code == _lib.BAD_CONFIG and "ShadowDataPointsFilter" in str(e.value)
        h.set_shadow(None)
        h.set_normals(None)
        h.set_covariance(0.01)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_shadow((None, 0.1))
        assert e.value.code == _lib.BAD_CONFIG and all(w in str(e.value) for w in both)
        assert h.shadow is None
        h.set_shadow((None, None))                                # no module on either side: nothing to refuse
    with icp.IcpHandle() as h:
        h.comm_init(0, 1, uid)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_shadow((None, 0.1))
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and "ShadowDataPointsFilter" in str(e.value)
        assert h.shadow is None


# ------------------------------------------------------------------------------------------------ CPU: the dump for upstream

def test_the_upstream_dump_emits_the_module(tmp_path):
    """devtools/dump_for_upstream.py on a chain with the module behind the sampling filter: reference_filtered.csv is what the
    host twin leaves of the oracle's filter output; the module on the reading is refused by name."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_for_upstream", os.path.join(ROOT, "devtools", "dump_for_upstream.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    doc = tmp_path / "chain.yaml"
    doc.write_text(cases.cases()["sampling"])
    rc, iterations = tool.dump(str(tmp_path / "dump"), 64, str(doc))
    assert rc == 0 and iterations > 0
    ref = synth.scan_pair(64)[0]
    rf, rn = icp.sampling_surface_normal(ref, 10, 0.5, 1)
    kp, kn = icp.shadow(rf, rn, 0.1)
    assert 10 <= len(kp) < len(rf)
    got = np.loadtxt(tmp_path / "dump" / "reference_filtered.csv", delimiter=",", skiprows=1, dtype=np.float64, ndmin=2).astype(F)
    assert np.array_equal(got[:, :3], kp[:, :3]) and np.array_equal(got[:, 3:6], kn)
    assert "41 Shadow" in (tmp_path / "dump" / "README.txt").read_text()
    doc.write_text(cases.cases()["reading"])
    with pytest.raises(SystemExit) as e:
        tool.dump(str(tmp_path / "rd"), 64, str(doc))
    assert "ShadowDataPointsFilter" in str(e.value)
