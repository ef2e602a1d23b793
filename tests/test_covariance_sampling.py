"""CovarianceSamplingDataPointsFilter: the host twin and the Jacobi against an independent numpy model
(tests/cov_sampling_model.py, written from the header's text), ties and degenerate clouds, what the module is for, the loader
through the C entry and both facades, the ABI's layout and symbols (CPU); the device entry against the host twin fed the
device's sums, the device's sums against the twin's own, and ICP.compute with the module against the same compute assembled
by hand, bit for bit (GPU).

The contract is in include/lsgpu_icp.h ("CovarianceSamplingDataPointsFilter").  Everything compares bits except the two
places that say otherwise: the Jacobi against numpy.linalg.eigh, and the device's tree-shaped double sums against the twin's
sequential ones."""
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
import cov_sampling_cases as cases
import cov_sampling_model as model
from cov_sampling_cases import PAIR_RD, PAIR_REF, RS, SN, SN_DENS, SN_RD, SNO, SSN, TRIM, chain, cov_sampling, max_density, shadow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "CovarianceSamplingDataPointsFilter"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return all(len(g) == len(w) and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ CPU: the host twin

@pytest.mark.parametrize("n", (7, 64, 65, 1000, 4099))
def test_host_twin_equals_the_model(n):
    p, v = cases.random_cloud(n)
    for nb in (1, 6, 7, n - 1):
        for tq in (0, 1, 2):
            got = icp.cov_sampling(p, v, nb, tq)
            want = model.cov_sampling(p, v, nb, tq)
            assert len(got[2]) == min(nb, n) and len(set(got[2].tolist())) == len(got[2]), (n, nb, tq)
            assert same(got, want), (n, nb, tq, got[2][:8], want[2][:8])
    for nb in (n, n + 1):                                        # the cloud comes back unchanged
        for tq in (0, 1, 2):
            got = icp.cov_sampling(p, v, nb, tq)
            assert same(got, (p, v, np.arange(n, dtype=np.int32))), (n, nb, tq)


def test_parameters_out_of_range_are_refused_by_the_twin():
    p, v = cases.random_cloud(64)
    for nb, tq in ((0, 1), (-1, 1), (2 ** 31 - 15, 1), (5, 3), (5, -1)):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.cov_sampling(p, v, nb, tq)
        assert e.value.code == _lib.BAD_CONFIG, (nb, tq)
    assert len(icp.cov_sampling(p, v, 2 ** 31 - 16, 1)[0]) == 64
    with pytest.raises(ValueError):
        icp.cov_sampling(p, v, 5.5, 1)
    k = C.c_int64(7)
    rc = _lib.lib().lsgpu_filter_cov_sampling(p.ctypes.data, v.ctypes.data, 64, 5, 1, None, p.ctypes.data, v.ctypes.data, None, C.byref(k), None)
    assert rc == _lib.BAD_ARG and k.value == 0                  # the outputs must not be the inputs


def test_twin_fed_its_own_sums_gives_the_same_result():
    p, v = cases.random_cloud(1000, seed=2)
    for tq in (0, 1, 2):
        *got, sums = icp.cov_sampling(p, v, 100, tq, return_sums=True)
        assert sums[31] == 1000 and (sums[9] != 0) == (tq == 1)
        c, L, vec, C21 = model.sums_and_vectors(p, v, tq)
        assert np.array_equal(sums[10:31], C21) and np.array_equal((sums[0:3] / 1000).astype(F), c)
        assert np.array_equal(sums[3:6], p[:, :3].min(axis=0).astype(np.float64)) and np.array_equal(sums[6:9], p[:, :3].max(axis=0).astype(np.float64))
        assert same(icp.cov_sampling(p, v, 100, tq, sums=sums), got)


# ------------------------------------------------------------------------------------------------ CPU: the Jacobi

def c21(M):
    return np.array([M[a, b] for a in range(6) for b in range(a, 6)], np.float64)


def test_jacobi_equals_the_model():
    mats = []
    for n, tq in ((64, 0), (1000, 1), (4099, 2)):
        p, v = cases.random_cloud(n, seed=3)
        mats.append(model.sums_and_vectors(p, v, tq)[3])
    p, v, _end = cases.corridor()
    mats.append(model.sums_and_vectors(p, v, 1)[3])
    mats.append(c21(np.diag([3.0, 1.0, 2.0, 1.0, 0.0, 5.0])))   # diagonal: no sweep, ties by the original column
    mats.append(c21(np.zeros((6, 6))))
    for m in mats:
        X, w = icp.cov_sampling_eigen(m)
        Xm, wm = model.jacobi(m)
        assert np.array_equal(bits(X), bits(Xm)) and np.array_equal(w, wm), m
        assert np.all(np.diff(w) >= 0)
    X, w = icp.cov_sampling_eigen(mats[-2])
    assert w.tolist() == [0.0, 1.0, 1.0, 2.0, 3.0, 5.0] and np.argmax(X, axis=0).tolist() == [4, 1, 3, 2, 0, 5]
    bad = mats[0].copy()
    bad[7] = np.nan
    with pytest.raises(_lib.LsgpuError) as e:
        icp.cov_sampling_eigen(bad)
    assert e.value.code == _lib.BAD_ARG


# Largest deviations measured on the inputs below (printed by the test): eigenvalues 1.82e-15 relative to the largest one,
# 1 - |X_k . E_k| 3.25e-8 (the rounding of X to float).  The tolerances are those times 16.
EIGH_VALUE_MEASURED, EIGH_VECTOR_MEASURED = 1.82e-15, 3.25e-8
EIGH_VALUE_TOL, EIGH_VECTOR_TOL = 16 * EIGH_VALUE_MEASURED, 16 * EIGH_VECTOR_MEASURED


def test_jacobi_against_eigh_on_spectra_with_gaps():
    rng = np.random.default_rng(11)
    worst_w = worst_v = 0.0
    for spectrum in ([1, 2, 4, 8, 16, 32], [0.5, 3, 10, 40, 900, 5000], [1e-3, 1, 7, 50, 51.5, 1e4], [2, 3, 5, 7, 11, 13]):
        for _ in range(8):
            Q, _r = np.linalg.qr(rng.normal(size=(6, 6)))
            M = (Q * np.array(spectrum, np.float64)) @ Q.T
            M = (M + M.T) / 2
            X, w = icp.cov_sampling_eigen(c21(M))
            we, E = np.linalg.eigh(M)
            worst_w = max(worst_w, float(np.max(np.abs(w - we)) / we[-1]))
            worst_v = max(worst_v, float(np.max(1.0 - np.abs(np.sum(X.astype(np.float64) * E, axis=0)))))
    print("jacobi vs eigh: eigenvalues %.3g (relative to the largest), 1 - |X.E| %.3g" % (worst_w, worst_v))
    assert worst_w <= EIGH_VALUE_TOL and worst_v <= EIGH_VECTOR_TOL


# ------------------------------------------------------------------------------------------------ CPU: ties, degenerate clouds

def test_duplicate_points_are_skipped_at_the_heads_and_tie_by_index():
    p, v = cases.random_cloud(40, seed=5)
    p, v = np.concatenate([p, p, p]), np.concatenate([v, v, v])  # every point three times: every magnitude ties three ways
    for tq in (0, 1, 2):
        for nb in (6, 50, 119):
            got = icp.cov_sampling(p, v, nb, tq)
            assert same(got, model.cov_sampling(p, v, nb, tq)), (tq, nb)
            ids = got[2]
            assert len(set(ids.tolist())) == nb
            for i in ids[ids >= 40]:                             # a copy is chosen only after the copies in front of it
                assert (i - 40) in ids[:list(ids).index(i)]


def test_one_plane_has_rank_three():
    rng = np.random.default_rng(6)
    p = np.ones((500, 4), F)
    p[:, :3] = np.stack([rng.uniform(-5, 5, 500), rng.uniform(-3, 3, 500), np.full(500, 2.0)], axis=1)
    v = np.tile(np.array([0, 0, 1], F), (500, 1))
    for tq in (0, 1, 2):
        C21 = model.sums_and_vectors(p, v, tq)[3]
        w = icp.cov_sampling_eigen(C21)[1]
        assert np.all(np.abs(w[:3]) <= 1e-12 * w[-1]) and np.all(w[3:] > 1e-3 * w[-1]), w
        for nb in (1, 7, 100):
            assert same(icp.cov_sampling(p, v, nb, tq), model.cov_sampling(p, v, nb, tq)), (tq, nb)


def test_degenerate_and_non_finite_clouds_are_bad_arg():
    p, v = cases.random_cloud(100, seed=7)
    same_pt = np.tile(p[:1], (100, 1))
    assert len(icp.cov_sampling(same_pt, v, 10, 0)[0]) == 10     # L = 1: nothing divides by the extent
    for tq in (1, 2):
        with pytest.raises(_lib.LsgpuError) as e:
            icp.cov_sampling(same_pt, v, 10, tq)
        assert e.value.code == _lib.BAD_ARG
        with pytest.raises(model.BadArg):
            model.cov_sampling(same_pt, v, 10, tq)
    for what in ("nan point", "inf normal", "inf point"):
        q, w = p.copy(), v.copy()
        if what == "nan point":
            q[17, 1] = np.nan
        elif what == "inf normal":
            w[99, 2] = np.inf
        else:
            q[0, 0] = -np.inf
        for tq in (0, 1, 2):
            o, on, oi = np.full((10, 4), 7, F), np.full((10, 3), 7, F), np.full(10, 7, np.int32)
            k = C.c_int64(5)
            rc = _lib.lib().lsgpu_filter_cov_sampling(q.ctypes.data, w.ctypes.data, 100, 10, tq, None, o.ctypes.data, on.ctypes.data,
                                                      oi.ctypes.data, C.byref(k), None)
            assert rc == _lib.BAD_ARG and k.value == 0, (what, tq)
            assert np.all(o == 7) and np.all(on == 7) and np.all(oi == 7)                      # the outputs are untouched
            with pytest.raises(model.BadArg):
                model.cov_sampling(q, w, 10, tq)


# ------------------------------------------------------------------------------------------------ CPU: what it is for

CORRIDOR_FACTOR = 10.0   # required; the model alone gives 30.4 on this cloud (80 of 200 kept points, 80 of 6080 in the cloud)


def test_a_corridor_keeps_its_end_wall():
    """A floor, two 40 m walls and an end wall holding 80 of 6080 points (1.3 %), nbSample 200, torqueNorm 0.  The model alone,
    on the CPU: 80 of the 200 kept points are end-wall points, 30.4 times their share of the cloud; the factor asked for is 10.
    (Shown by the model too and not asserted: at torqueNorm 1 and 2 the torque components shrink by Lnorm ~ 10 and ~ 20, the
    least constrained direction becomes the rotation about the corridor's axis, which no single point constrains by more than
    0.02 per pick, and the factor is 1.5 and 0.4 -- the walk as stated serves that direction with nearly every pick.)"""
    p, v, end = cases.corridor()
    assert len(p) == 6080 and end.sum() == 80
    share = end.mean()
    ids_m = model.cov_sampling(p, v, 200, 0)[2]
    print("corridor: model's end-wall share among the kept %.3f, in the cloud %.4f, factor %.1f" % (end[ids_m].mean(), share, end[ids_m].mean() / share))
    assert end[ids_m].mean() / share > 3 * CORRIDOR_FACTOR
    ids = icp.cov_sampling(p, v, 200, 0)[2]
    assert end[ids].mean() >= CORRIDOR_FACTOR * share
    assert np.array_equal(ids, ids_m)


# ------------------------------------------------------------------------------------------------ CPU: the loader

COV = "PointToPlaneWithCovErrorMinimizer"
# documents that load -> ((reading nbSample, torqueNorm) or None, the same of the reference)
ACCEPTED = [
    (chain(reading=RS + SN_RD + cov_sampling(800, 2) + PAIR_RD, reference=SSN + cov_sampling(600, 0) + PAIR_REF, outliers=TRIM + SNO), ((800, 2), (600, 0))),
    (chain(reading=RS + SN_RD + PAIR_RD + cov_sampling(800), reference=SN + PAIR_REF + cov_sampling(tq=2), outliers=TRIM + SNO), ((800, 1), (5000, 2))),
    # behind MaxDensityDataPointsFilter and ShadowDataPointsFilter
    (chain(reading=RS + SN_RD + shadow("0.25") + cov_sampling(100, 1), reference=SN_DENS + max_density("50") + shadow("0.2") + cov_sampling(2147483632, 1) + PAIR_REF,
           outliers=TRIM + SNO), ((100, 1), (2147483632, 1))),
    (chain(reference=SN_DENS + max_density("50") + PAIR_REF + cov_sampling(1, 0)), (None, (1, 0))),
    # the defaults; a point-to-point chain (the normals are computed for the module)
    (chain(reference=SSN + cov_sampling()), (None, (5000, 1))),
    (chain(reference=SN + cov_sampling("5e2", "2.0"), minimizer="PointToPointErrorMinimizer"), (None, (500, 2))),
]
# (document, words the refusal must hold)
REFUSALS = [
    # in front of the section's normals module; a section without one
    (chain(reference=cov_sampling() + SSN), (NAME, "needs the normals")),
    (chain(reading=RS + cov_sampling() + SN_RD, outliers=TRIM + SNO), (NAME, "needs the normals")),
    (chain(reading=cov_sampling() + RS), (NAME, "needs the normals")),
    (chain(reference=cov_sampling(), minimizer="PointToPointErrorMinimizer"), (NAME, "needs the normals")),
    (chain(reading=RS + cov_sampling(), outliers=TRIM + SNO), (NAME, "needs the normals")),
    # inside the orientation pair
    (chain(reference=SSN + PAIR_REF.replace("  - OrientNormals", cov_sampling() + "  - OrientNormals")), (NAME, "between")),
    (chain(reading=RS + SN_RD + "  - ObservationDirectionDataPointsFilter\n" + cov_sampling() + "  - OrientNormalsDataPointsFilter\n", outliers=TRIM + SNO),
     (NAME, "between")),
    # in front of the section's MaxDensity- or ShadowDataPointsFilter
    (chain(reference=SN_DENS + cov_sampling() + max_density("50")), (NAME, "in front of MaxDensityDataPointsFilter")),
    (chain(reference=SSN + cov_sampling() + shadow()), (NAME, "in front of ShadowDataPointsFilter")),
    (chain(reading=RS + SN_RD + cov_sampling() + shadow(), outliers=TRIM + SNO), (NAME, "in front of ShadowDataPointsFilter")),
    # parameters
    (chain(reference=SSN + cov_sampling(0)), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling(-5)), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling(2147483633)), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling("7.5")), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling("abc")), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling(".inf")), (NAME, "nbSample")),
    (chain(reference=SSN + cov_sampling(tq=3)), (NAME, "torqueNorm")),
    (chain(reference=SSN + cov_sampling(tq=-1)), (NAME, "torqueNorm")),
    (chain(reference=SSN + cov_sampling(tq="0.5")), (NAME, "torqueNorm")),
    (chain(reference=SSN + cov_sampling(5) + "      bogus: 1\n"), (NAME, "bogus")),
    # a second instance
    (chain(reference=SSN + cov_sampling() + cov_sampling()), (NAME, "twice")),
    (chain(reading=RS + SN_RD + cov_sampling() + cov_sampling(), outliers=TRIM + SNO), (NAME, "twice")),
    # together with the covariance minimizer
    (chain(reference=SSN + cov_sampling(), minimizer=COV), (COV, NAME)),
    # on the reading of a chain without SurfaceNormalOutlierFilter
    (chain(reading=RS + SN_RD + cov_sampling()), (NAME, "SurfaceNormalOutlierFilter")),
]


def _load(text):
    doc = yaml.load(text, Loader=yaml.BaseLoader) or {}
    return icp.chain_load(doc), icp.chain_load_cuts(doc), icp.chain_load_shadow(doc), icp.chain_load_motion(doc), icp.chain_load_cov_sampling(doc)


@pytest.fixture(scope="module")
def cpp_lines(tmp_path_factory):
    """tests/cpp/cov_sampling_loader_check.cpp over ACCEPTED and REFUSALS -> (its lines, its LAYOUT line)"""
    tmp = tmp_path_factory.mktemp("cov_sampling_loader")
    exe, docs = str(tmp / "cov_sampling_loader_check"), str(tmp / "docs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "cov_sampling_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    texts = [d for d, _ in ACCEPTED] + [d for d, _ in REFUSALS]
    with open(docs, "wb") as f:
        for t in texts:
            b = t.encode()
            f.write(b"DOC %d\n" % len(b) + b)
    r = subprocess.run([exe, docs], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "cov_sampling_loader_check: ok %d" % len(texts), r.stdout[-2000:] + r.stderr
    assert lines[-2].startswith("LAYOUT ")
    return lines[:-2], lines[-2]


def _word(pair):
    return "-" if pair is None else "%d,%d" % pair


def test_documents_with_the_module_load_through_the_c_entry_and_both_facades(cpp_lines):
    """Fails without the feature: the commit before refuses every one of these documents with "referenceDataPointsFilters:
    module CovarianceSamplingDataPointsFilter is not implemented on the HIP path" (or readingDataPointsFilters)."""
    for (text, (rd, ref)), line in zip(ACCEPTED, cpp_lines[0]):
        loads = _load(text)
        assert all(r[0] == _lib.OK for r in loads), (text, [r[1] for r in loads])
        (_rc, _why, lc), (_rc2, _why2, cc) = loads[0], loads[1]
        cs = loads[4][2]
        assert (cs.reading_nb_sample, cs.reading_torque_norm) == (rd or (0, 1)) and (cs.reference_nb_sample, cs.reference_torque_norm) == (ref or (0, 1)), text
        assert tuple(cs.reserved) == (0, 0, 0, 0)
        o = icp.ICP()
        o.load_from_yaml(io.StringIO(text))
        assert o.chain.cov_sampling == (rd, ref)
        assert line == "OK %s %s %s %s" % (_word(rd), _word(ref), bytes(lc).hex(), bytes(cc).hex()), text
    # the document without the module next to one with it: the same lsgpu_loaded_chain
    with_m = ACCEPTED[0][0]
    without = with_m.replace(cov_sampling(800, 2), "").replace(cov_sampling(600, 0), "")
    assert NAME not in without and bytes(_load(with_m)[0][2]) == bytes(_load(without)[0][2])
    cs = _load(without)[4][2]
    assert (cs.reading_nb_sample, cs.reference_nb_sample, cs.reading_torque_norm, cs.reference_torque_norm) == (0, 0, 1, 1)
    assert icp.ICP().chain.cov_sampling is None


def test_refusals_name_the_module_through_the_c_entry_and_both_facades(cpp_lines, tmp_path):
    lines = cpp_lines[0][len(ACCEPTED):]
    assert len(lines) == len(REFUSALS)
    for (text, words), line in zip(REFUSALS, lines):
        loads = _load(text)
        whys = {r[1] for r in loads}
        assert all(r[0] == _lib.BAD_CONFIG for r in loads) and len(whys) == 1, (text, whys)
        why = whys.pop()
        for w in words:
            assert w in why, (text, why)
        with pytest.raises(_lib.LsgpuError) as e:
            icp.ICP().load_from_yaml(io.StringIO(text))
        assert e.value.code == _lib.BAD_CONFIG and why in str(e.value)
        assert line == "ERR " + why, (text, line)
    _input_filter_chain_refuses_the_name(tmp_path)
    # the reading's module reached while the reference's keepDensities 1 still waits for its MaxDensityDataPointsFilter: the
    # densities' own rule answers, not a text about the reading standing in front of MaxDensityDataPointsFilter
    text = ("referenceDataPointsFilters:\n" + SN_DENS + "readingDataPointsFilters:\n" + RS + SN_RD + cov_sampling()
            + chain(reading="", reference="", outliers=TRIM + SNO))
    loads = _load(text)
    assert all(r[0] == _lib.BAD_CONFIG for r in loads) and len({r[1] for r in loads}) == 1
    assert "keepDensities 1" in loads[0][1] and "readingDataPointsFilters" not in loads[0][1], loads[0][1]


def _input_filter_chain_refuses_the_name(tmp_path):
    """LaserTrack's input filter chain (DataPointsFilters of the C++ facade): the name stays unknown."""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cstdio>\n#include <sstream>\n#include "laser_slam_amd/icp.hpp"\n'
                   'int main() { std::istringstream y("- CovarianceSamplingDataPointsFilter:\\n    nbSample: 10\\n");\n'
                   '  try { laser_slam_amd::DataPointsFilters f(y); } catch (const std::exception& e) { std::printf("ERR %s\\n", e.what()); return 0; }\n'
                   '  std::printf("LOADED\\n"); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           str(src), "-o", exe, "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout
    assert out.startswith("ERR ") and NAME in out, out


# ------------------------------------------------------------------------------------------------ CPU: the ABI

def test_struct_layout_symbols_and_abi_version(cpp_lines):
    L = _lib.lib()
    S = _lib.CovSamplingCfg
    layout = [int(x) for x in cpp_lines[1].split()[1:]]
    assert layout == [C.sizeof(S), S.reading_nb_sample.offset, S.reference_nb_sample.offset, S.reading_torque_norm.offset,
                      S.reference_torque_norm.offset, S.reserved.offset] == [32, 0, 4, 8, 12, 16]
    assert L.lsgpu_abi_version() == 4
    with open(os.path.join(ROOT, "include", "lsgpu_icp.h")) as f:
        header = f.read()
    assert "#define LSGPU_ABI_VERSION 4\n" in header
    names = set(re.findall(r"\b(lsgpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))   # every function the header names
    new = {"lsgpu_cov_sampling_config_default", "lsgpu_cov_sampling_config_check", "lsgpu_cov_sampling_config_why",
           "lsgpu_icp_set_cov_sampling", "lsgpu_icp_filter_cov_sampling", "lsgpu_filter_cov_sampling", "lsgpu_cov_sampling_eigen",
           "lsgpu_chain_load_cov_sampling", "lsgpu_icp_cov_sampling_phase_ms"}
    assert new <= names and len(names) > 85
    for name in sorted(names):
        assert hasattr(L, name), name
    assert new <= set(_lib.ABI_SYMBOLS)
    c = S()
    c.reading_nb_sample = c.reference_torque_norm = 9
    c.reserved[2] = 9
    L.lsgpu_cov_sampling_config_default(C.byref(c))
    assert (c.reading_nb_sample, c.reference_nb_sample, c.reading_torque_norm, c.reference_torque_norm, tuple(c.reserved)) == (0, 0, 1, 1, (0, 0, 0, 0))
    assert L.lsgpu_cov_sampling_config_check(C.byref(c)) == _lib.OK and L.lsgpu_cov_sampling_config_why(C.byref(c)) is None
    for rd, ref, tr, tf, ok, word in ((5000, 0, 1, 1, True, None), (0, 2 ** 31 - 16, 0, 2, True, None), (1, 1, 2, 0, True, None),
                                      (-1, 0, 1, 1, False, b"nbSample"), (0, 2 ** 31 - 15, 1, 1, False, b"nbSample"),
                                      (5, 5, 3, 1, False, b"torqueNorm"), (5, 5, 1, -1, False, b"torqueNorm")):
        c.reading_nb_sample, c.reference_nb_sample, c.reading_torque_norm, c.reference_torque_norm = rd, ref, tr, tf
        assert (L.lsgpu_cov_sampling_config_check(C.byref(c)) == _lib.OK) == ok, (rd, ref, tr, tf)
        why = L.lsgpu_cov_sampling_config_why(C.byref(c))
        assert (why is None) == ok and (ok or (NAME.encode() in why and word in why))
    c.reading_nb_sample, c.reference_nb_sample, c.reading_torque_norm, c.reference_torque_norm = 5, 5, 1, 1
    c.reserved[3] = 1
    assert L.lsgpu_cov_sampling_config_check(C.byref(c)) == _lib.BAD_CONFIG
    assert L.lsgpu_cov_sampling_config_check(None) == _lib.BAD_CONFIG


# ------------------------------------------------------------------------------------------------ GPU: the device entry

@pytest.fixture(scope="module")
def handle():
    with icp.IcpHandle() as h:
        yield h


@pytest.mark.gpu
@pytest.mark.parametrize("n", (63, 64, 65, 257, 4099, 70001))
def test_device_entry_equals_the_host_twin_fed_the_devices_sums(n, handle):
    """Wave and block edges of the sums passes, the sort and the gather; 70 001: 274 blocks of the sums passes (the final pass
    combines more rows than it has groups) and 69 blocks of the sort with a ragged last one.  Host pointers, and device pointers
    once per size.  Two runs give the same bytes."""
    import torch
    p, v = cases.random_cloud(n, seed=1)
    for nb in (1, 64, 65, n - 1):
        for tq in (0, 1, 2):
            *got, sums = handle.filter_cov_sampling(p, v, nb, tq, return_sums=True)
            assert len(got[2]) == min(nb, n)
            want = icp.cov_sampling(p, v, nb, tq, sums=sums)
            assert same(got, want), (n, nb, tq, got[2][:8], want[2][:8])
            *again, sums2 = handle.filter_cov_sampling(p, v, nb, tq, return_sums=True)
            assert same(again, got) and sums.tobytes() == sums2.tobytes(), (n, nb, tq)
    dp, dv = torch.from_numpy(p).cuda(), torch.from_numpy(v).cuda()
    got = handle.filter_cov_sampling(dp, dv, 64, 1)
    assert all(g.is_cuda for g in got)
    assert same([g.cpu().numpy() for g in got], handle.filter_cov_sampling(p, v, 64, 1)), n
    assert np.array_equal(bits(dp.cpu().numpy()), bits(p)) and np.array_equal(bits(dv.cpu().numpy()), bits(v))   # the inputs are only read


@pytest.mark.gpu
def test_device_entry_on_tied_magnitudes_and_chosen_heads(handle):
    """Every point three times: every magnitude ties three ways, so the radix sort's stability decides the order inside a list
    (ascending index) and the walk meets heads that are already chosen.  Against the twin fed the device's sums, bit for bit."""
    p, v = cases.random_cloud(40, seed=5)
    p, v = np.concatenate([p, p, p]), np.concatenate([v, v, v])
    for tq in (0, 1, 2):
        for nb in (6, 50, 119):
            *got, sums = handle.filter_cov_sampling(p, v, nb, tq, return_sums=True)
            assert same(got, icp.cov_sampling(p, v, nb, tq, sums=sums)), (tq, nb)
            ids = got[2]
            assert len(set(ids.tolist())) == nb
            for i in ids[ids >= 40]:                             # a copy is chosen only after the copies in front of it
                assert (i - 40) in ids[:list(ids).index(i)]


def _sequential_and_abs(p, v, tq, S=None, len_sum=None):
    """The 25 double sums added sequentially by the model (S and the sum of lengths taken as given where they are given, so that
    every term behind them is the device's term), and the sum of |terms| of each -> (32 doubles, 32 doubles)"""
    c, L, vec, C21 = model.sums_and_vectors(p, v, tq, S, len_sum)
    seq, mag = np.zeros(32), np.zeros(32)
    pd = p[:, :3].astype(np.float64)
    seq[0:3] = [np.cumsum(pd[:, a])[-1] for a in range(3)]
    mag[0:3] = np.abs(pd).sum(axis=0)
    if tq == 1:
        d = p[:, :3] - c
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float64)
        seq[9], mag[9] = np.cumsum(ln)[-1], ln.sum()
    vd = vec.astype(np.float64)
    seq[10:31] = C21
    mag[10:31] = [np.abs(vd[:, a] * vd[:, b]).sum() for a in range(6) for b in range(a, 6)]
    return seq, mag


@pytest.mark.gpu
@pytest.mark.parametrize("n", (4099, 70001))
def test_device_sums_are_within_the_reordering_bound_of_the_twins(n, handle):
    """Each double sum of the device within n 2^-52 sum|terms| of the sequential sum of the same terms: the bound for
    reordering a double sum of exactly representable terms (each of the n - 1 additions of either order is off by at most
    2^-53 of a partial sum, and no partial sum exceeds sum|terms|) -- derived, not measured.  Minimum, maximum and n are exact.
    S is compared with the twin's own.  The terms of the sum of lengths hold c = (float)(S / n), those of C hold c and Lnorm:
    where the device's S rounds to another c than the twin's, the twin's terms are other numbers, not the same numbers in
    another order, so these sums are compared with the sequential sum of the DEVICE's terms (the model fed the device's S
    and sum of lengths: the twin's arithmetic, as the CPU tests show) -- and with the twin's own as well where c and Lnorm agree."""
    p, v = cases.random_cloud(n, seed=1)
    for tq in (0, 1, 2):
        *dev, sd = handle.filter_cov_sampling(p, v, 64, tq, return_sums=True)
        *own, st = icp.cov_sampling(p, v, 64, tq, return_sums=True)
        assert np.array_equal(sd[3:9], st[3:9]) and sd[31] == st[31] == n
        seq, mag = _sequential_and_abs(p, v, tq, S=sd[0:3], len_sum=sd[9] if tq == 1 else None)
        bound = n * 2.0 ** -52 * mag
        err = np.abs(sd - np.concatenate([st[0:3], seq[3:]]))
        print("n %d torqueNorm %d: largest error / bound %.3g" % (n, tq, np.max(err[[0, 1, 2] + list(range(9, 31))] / np.maximum(bound[[0, 1, 2] + list(range(9, 31))], 1e-300))))
        assert np.all(err[0:3] <= bound[0:3]) and err[9] <= bound[9] and np.all(err[10:31] <= bound[10:31]), (n, tq, err, bound)
        same_c = np.array_equal((sd[0:3] / n).astype(F), (st[0:3] / n).astype(F))
        if same_c and tq == 1:
            assert abs(sd[9] - st[9]) <= bound[9], (n, tq)
        if same_c and (tq != 1 or F(sd[9] / n) == F(st[9] / n)):
            assert np.all(np.abs(sd[10:31] - st[10:31]) <= bound[10:31]), (n, tq)
        print("n %d torqueNorm %d: c and Lnorm equal the twin's: %s; kept list with the twin's own sums equals the device's: %s"
              % (n, tq, same_c, same(dev, own)))


@pytest.mark.gpu
def test_edges_and_error_codes_of_the_device_entry(handle):
    p, v = cases.random_cloud(300, seed=8)
    for nb in (300, 301, 2 ** 31 - 16):                          # nbSample >= n: the input comes back
        assert same(handle.filter_cov_sampling(p, v, nb, 1), (p, v, np.arange(300, dtype=np.int32)))
    for nb, tq, word in ((0, 1, "nbSample"), (2 ** 31 - 15, 1, "nbSample"), (5, 3, "torqueNorm")):
        with pytest.raises(_lib.LsgpuError) as e:
            handle.filter_cov_sampling(p, v, nb, tq)
        assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value) and word in str(e.value)
    same_pt = np.tile(p[:1], (300, 1))
    assert len(handle.filter_cov_sampling(same_pt, v, 10, 0)[0]) == 10
    q = p.copy()
    q[123, 2] = np.nan
    w = v.copy()
    w[299, 0] = np.inf
    for args in ((same_pt, v, 10, 1), (same_pt, v, 10, 2), (q, v, 10, 0), (q, v, 10, 1), (p, w, 10, 2)):
        o, on, oi = np.full((10, 4), 7, F), np.full((10, 3), 7, F), np.full(10, 7, np.int32)
        k = C.c_int64(5)
        rc = _lib.lib().lsgpu_icp_filter_cov_sampling(handle._h, args[0].ctypes.data, args[1].ctypes.data, 300, args[2], args[3], o.ctypes.data,
                                                      on.ctypes.data, oi.ctypes.data, C.byref(k), None)
        assert rc == _lib.BAD_ARG and k.value == 0 and NAME.encode() in _lib.lib().lsgpu_last_error(handle._h)
        assert np.all(o == 7) and np.all(on == 7) and np.all(oi == 7)                          # the outputs are untouched
    k = C.c_int64(0)
    rc = _lib.lib().lsgpu_icp_filter_cov_sampling(handle._h, p.ctypes.data, v.ctypes.data, 300, 10, 1, p.ctypes.data, v.ctypes.data, None, C.byref(k), None)
    assert rc == _lib.BAD_ARG
    assert same(handle.filter_cov_sampling(p, v, 10, 1), icp.cov_sampling(p, v, 10, 1, sums=handle.filter_cov_sampling(p, v, 10, 1, return_sums=True)[3]))


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


SIDES = {"sampling": ("reference",), "surface_normal": ("reference",), "max_density": ("reference", "reference MaxDensity"),
         "shadow": ("reference", "reference Shadow"), "point_to_point": ("reference",), "reading": ("reading",),
         "both": ("reference", "reading"), "sn_shadow": ("reference", "reference Shadow"),
         "sn_max_density_shadow": ("reference", "reference MaxDensity", "reference Shadow"),
         "sn_max_density_point_to_point": ("reference MaxDensity",), "sn_shadow_point_to_point": ("reference", "reference Shadow")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIDES))
def test_compute_with_the_module_equals_the_compute_by_hand(name, pair):
    """Route a: the loaded document through the Python facade, end to end.  Route b: the kernel-level entries, the module by
    lsgpu_icp_filter_cov_sampling, set_reference + align / align_normals.  T_out, the stats' result fields, the whole trace, the
    reference the handle holds and the draw stream: equal."""
    a, pos_a = route_a(name, pair)
    b, pos_b, counts = cases.route_b(cases.cases()[name], pair["rd"], pair["ref"], pair["T_init"])
    print(name, "handed to the module / kept:", counts, "iterations", a[1])
    assert tuple(sorted(counts)) == tuple(sorted(SIDES[name]))
    for side, (n_in, kept) in counts.items():                   # a module that drops nothing shows nothing
        assert kept < n_in, (name, side, n_in, kept)
    assert a[1] >= 3 and len(a[5]) > 0
    assert a[0] == b[0], (np.frombuffer(a[0], F), np.frombuffer(b[0], F))                           # T_out
    assert a[1:5] == b[1:5]                                                                       # iterations, converged, final limit, final n_used
    assert a[5] == b[5]                                                                           # the trace
    assert a[6] == b[6] and ("reference" not in counts or a[6] == counts["reference"][1])         # the reference the handle holds
    assert pos_a == pos_b                                                                         # the draw stream


@pytest.mark.gpu
def test_compute_without_the_side_stream(pair):
    """LSGPU_NO_SIDE_STREAM=1 (read once per process: a fresh child): a chain whose reading runs on the side stream, both routes
    in the child, against route a of this process."""
    env = dict(os.environ, LSGPU_NO_SIDE_STREAM="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cov_sampling_cases.py")], env=env, capture_output=True, text=True, timeout=120)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("COV_SAMPLING_RESULT ")]
    assert r.returncode == 0 and line, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(line[0][len("COV_SAMPLING_RESULT "):])
    assert set(res) == set(cases.SIDE_CASES)
    for name in cases.SIDE_CASES:
        assert res[name]["a"] == res[name]["b"] == cases.digest(*route_a(name, pair)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("plain", "point_to_point", "cut"))
def test_an_nb_sample_that_reaches_the_section_equals_the_document_without_the_module(name, pair):
    """SurfaceNormalDataPointsFilter with the module alone behind it, nbSample at and above what the module would be handed: the
    section passes unchanged and the compute is the one of the document without the module -- T_out, the stats' result fields,
    the trace, the reference the handle holds and the draw stream, bit for bit.  "cut": a MaxDist module in front leaves 3226 of
    the 4096 points and nbSample lies between the two, so it is the count behind the cut that it reaches.  (Which grid the
    normals are computed on is the plan's decision and changes no result: tests/cpp/section_plan_check.cpp pins it.)"""
    rd, ref, T_init = pair["rd"], pair["ref"], pair["T_init"]
    n_handed = 4096
    if name == "cut":
        n_handed = int((np.linalg.norm(ref[:, :3].astype(np.float64), axis=1) < 10).sum())
        assert n_handed == 3226
    without = None
    for nb in ((3226, 3600) if name == "cut" else (4096, 6000)):
        assert n_handed <= nb and (name != "cut" or nb < 4096)
        doc, doc_without = cases.fallback_cases(nb)[name]
        if without is None:
            without = cases.route_a(doc_without, rd, ref, T_init)
        a, pos_a = cases.route_a(doc, rd, ref, T_init)
        assert a[1] >= 3 and len(a[5]) > 0 and a[6] == n_handed
        assert (a, pos_a) == without, (name, nb)


def _default_result(h, pair):
    T, st = h.compute(pair["rd"], pair["ref"], pair["T_init"], 0.5, 10, 0.5, 11)
    return T.tobytes(), int(st.iterations), int(st.final_n_used), cases.trace_bytes(h)


def _sn_result(h, pair):
    T, st = h.compute(pair["rd"], pair["ref"], pair["T_init"], 0.5, 0, 0.5, 11, sn_knn=10)
    return T.tobytes(), int(st.iterations), int(st.final_n_used), cases.trace_bytes(h)


@pytest.mark.gpu
def test_a_degenerate_or_emptied_section_is_an_error_that_leaves_the_handle_usable(pair):
    """The module's error returns inside compute.  Degenerate: every point of the section the same, Lnorm 0 at torqueNorm 1 and
    2 -- on the reference by the SurfaceNormalDataPointsFilter route, on the reading behind its normals.  Emptied: a Shadow pass
    in front that drops everything (|cos| <= 1 < 3.1416).  Each is the error the header names, and the same handle with the
    modules removed then gives the fresh handle's T and trace."""
    rd, ref, T_init = pair["rd"], pair["ref"], pair["T_init"]
    with icp.IcpHandle() as h:
        fresh = _default_result(h, pair)
    flat_ref, flat_rd = np.tile(ref[:1], (400, 1)), np.tile(rd[:1], (400, 1))
    with icp.IcpHandle() as h:
        for tq in (1, 2):
            h.set_cov_sampling((None, (100, tq)))
            with pytest.raises(_lib.LsgpuError) as e:
                h.compute(rd, flat_ref, T_init, 0.5, 0, 0.5, 11, sn_knn=10)
            assert e.value.code == _lib.BAD_ARG and NAME in str(e.value) and "Lnorm" in str(e.value), (tq, str(e.value))
            h.set_cov_sampling(None)
            assert _default_result(h, pair) == fresh, tq
    nc = icp.NormalsConfig(0.6, 7, 1, 1)
    with icp.IcpHandle(normals=nc) as h:
        for tq in (1, 2):
            h.set_cov_sampling(((50, tq), None))
            with pytest.raises(_lib.LsgpuError) as e:
                h.compute(flat_rd, ref, T_init, 0.5, 10, 0.5, 11)
            assert e.value.code == _lib.BAD_ARG and NAME in str(e.value) and "Lnorm" in str(e.value), (tq, str(e.value))
        h.set_cov_sampling(None)
        h.set_normals(None)
        assert _default_result(h, pair) == fresh
    with icp.IcpHandle(shadow=(None, 3.1416), cov_sampling=(None, (100, 1))) as h:
        for kw in (dict(ssn_knn=10), dict(ssn_knn=0, sn_knn=10)):
            with pytest.raises(_lib.ConvergenceError) as e:
                h.compute(rd, ref, T_init, 0.5, seed=11, **kw)
            assert "the reference filter left no point" in str(e.value)
        h.set_shadow(None)
        h.set_cov_sampling(None)
        assert _default_result(h, pair) == fresh
    with icp.IcpHandle(normals=nc, shadow=(3.1416, None), cov_sampling=((50, 1), None)) as h:
        with pytest.raises(_lib.ConvergenceError) as e:
            h.compute(rd, ref, T_init, 0.5, 10, 0.5, 11)
        assert "the reading filter left no point" in str(e.value)
        h.set_cov_sampling(None)
        h.set_shadow(None)
        h.set_normals(None)
        assert _default_result(h, pair) == fresh


@pytest.mark.gpu
def test_the_module_on_a_handle_comes_and_goes(pair):
    rd, ref, T_init = pair["rd"], pair["ref"], pair["T_init"]
    with icp.IcpHandle() as h:
        fresh = _default_result(h, pair)
    with icp.IcpHandle(cov_sampling=(None, (100, 1))) as h:
        # a section with no more than nbSample points passes unchanged; removing the module gives the trace of a plain handle
        h.set_cov_sampling((None, (4096, 1)))
        assert _default_result(h, pair) == fresh
        h.set_cov_sampling((None, (100, 1)))
        assert _default_result(h, pair) != fresh
        h.set_cov_sampling(None)
        assert h.cov_sampling is None and _default_result(h, pair) == fresh
    # behind SurfaceNormalDataPointsFilter alone, nbSample >= n: what a handle without the module gives
    with icp.IcpHandle() as h:
        plain = _sn_result(h, pair)
        for nb, tq in ((4096, 1), (5000, 2)):
            h.set_cov_sampling((None, (nb, tq)))
            assert _sn_result(h, pair) == plain, (nb, tq)
        h.set_cov_sampling((None, (1500, 1)))
        assert _sn_result(h, pair) != plain
    # the module on a chain with no reference normals: refused by name
    with icp.IcpHandle(error_minimizer="PointToPointErrorMinimizer", cov_sampling=(None, (100, 1))) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.compute(rd, ref, T_init, 0.5, 0, 0.5, 11)
        assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value)


@pytest.mark.gpu
def test_refusals_on_the_handle_in_either_order():
    """A GPU test because lsgpu_icp_create opens the device: without one there is no handle to refuse anything."""
    uid = icp.comm_unique_id()
    both = (COV, NAME)
    with icp.IcpHandle() as h:
        h.set_cov_sampling((None, (100, 1)))
        assert h.cov_sampling == (None, (100, 1))
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_covariance(0.01)
        assert e.value.code == _lib.BAD_CONFIG and all(w in str(e.value) for w in both)
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, uid)
        assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value)
        for bad in ((None, (-3, 1)), (None, (100, 3)), ((2 ** 31 - 15, 1), None)):      # a bad value: the handle keeps what it had
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_cov_sampling(bad)
            assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value)
        assert h.cov_sampling == (None, (100, 1)) and h.covariance is None
        # the reading's module without the reading's normals
        for normals in (None, icp.NormalsConfig(0.6, reading_normals_given=1)):
            h.set_normals(normals)
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_cov_sampling(((100, 1), None))
            assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value) and "SurfaceNormalDataPointsFilter" in str(e.value)
        # ... and the other order: the normals may not leave while the reading's module is on
        h.set_normals(icp.NormalsConfig(0.6, 7, 0, 0))
        h.set_cov_sampling(((100, 1), None))
        for normals in (None, icp.NormalsConfig(0.6, reading_normals_given=1)):
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_normals(normals)
            assert e.value.code == _lib.BAD_CONFIG and NAME in str(e.value)
        h.set_cov_sampling(None)
        h.set_normals(None)
        h.set_covariance(0.01)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_cov_sampling((None, (100, 1)))
        assert e.value.code == _lib.BAD_CONFIG and all(w in str(e.value) for w in both)
        assert h.cov_sampling is None
        h.set_cov_sampling((None, None))                          # no module on either side: nothing to refuse
    with icp.IcpHandle() as h:
        h.comm_init(0, 1, uid)
        with pytest.raises(_lib.LsgpuError) as e:
            h.set_cov_sampling((None, (100, 1)))
        assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and NAME in str(e.value)
        assert h.cov_sampling is None


# ------------------------------------------------------------------------------------------------ CPU: the dump for upstream

def test_the_upstream_dump_emits_the_module(tmp_path):
    """devtools/dump_for_upstream.py on a chain with the module behind the sampling filter: reference_filtered.csv is what the
    host twin picks of the oracle's filter output, in pick order; the module on the reading is refused by name."""
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
    kp, kn, _ids = icp.cov_sampling(rf, rn, 600, 1)
    assert len(kp) == 600 < len(rf)
    got = np.loadtxt(tmp_path / "dump" / "reference_filtered.csv", delimiter=",", skiprows=1, dtype=np.float64, ndmin=2).astype(F)
    assert np.array_equal(got[:, :3], kp[:, :3]) and np.array_equal(got[:, 3:6], kn)
    assert "55 CovarianceSampling" in (tmp_path / "dump" / "README.txt").read_text()
    doc.write_text(cases.cases()["reading"])
    with pytest.raises(SystemExit) as e:
        tool.dump(str(tmp_path / "rd"), 64, str(doc))
    assert NAME in str(e.value)
