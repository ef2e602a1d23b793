"""PointToPlaneErrorMinimizer force2D / force4DOF and BoundTransformationChecker: the loader through the three front ends, the
host twins against a float64 restatement, the ABI's layout and symbols (CPU); the sums, the loop against the host, the
constraint itself, the bound and the neutrality of a handle that had the modules (GPU).

The contract is in include/lsgpu_icp.h ("PointToPlaneErrorMinimizer force4DOF / force2D and BoundTransformationChecker").
The GPU tests search, move and select with the library's kernel-level entries (lsgpu_knn, lsgpu_transform_points,
lsgpu_trim_limit: exact, held against the oracle elsewhere) and form the sums and the steps on the host."""
import ctypes as C
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import yaml

from laser_slam_amd import _lib, icp, synth
import motion_cases as mc
from motion_cases import COUNTER, DIFF, DOF_3, DOF_4, DOF_6, MAXD, MEDIAN, MIND, ROBUST, SN_RD, SNO, TRIM, bound, chain, minimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EPS32 = float(np.finfo(F).eps)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ CPU: the loader

# (document, (dof, bound, maxRotationNorm, maxTranslationNorm, bound_before_counter))
ACCEPTED = [
    (chain(minimizer(force2D=1)), (DOF_3, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force4DOF=1)), (DOF_4, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force2D=1, force4DOF=0)), (DOF_3, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force2D=1), outliers=TRIM + MAXD), (DOF_3, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force4DOF=1), outliers=MIND), (DOF_4, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force2D=1), outliers=MEDIAN), (DOF_3, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force4DOF=1), outliers=TRIM + MAXD + MIND + MEDIAN, max_dist="2.5"), (DOF_4, 0, 1.0, 1.0, 0)),
    (chain(minimizer(force2D=1), outliers=""), (DOF_3, 0, 1.0, 1.0, 0)),
    (chain(checkers=bound("0.5", "2") + COUNTER + DIFF), (DOF_6, 1, 0.5, 2.0, 1)),             # in front of the counter
    (chain(checkers=COUNTER + bound("0.5", "2") + DIFF), (DOF_6, 1, 0.5, 2.0, 0)),             # behind it
    (chain(checkers=COUNTER + DIFF + bound()), (DOF_6, 1, 1.0, 1.0, 0)),                       # the module's defaults
    (chain(checkers=COUNTER + bound(trans="0")), (DOF_6, 1, 1.0, 0.0, 0)),
    (chain(minimizer(force4DOF=1), checkers=bound("0.1") + COUNTER), (DOF_4, 1, 0.1, 1.0, 1)),
    (chain(minimizer("PointToPointErrorMinimizer"), checkers=COUNTER + bound(), reference=""), (DOF_6, 1, 1.0, 1.0, 0)),
    # every other parameter of PointToPlaneErrorMinimizer stays "not looked at"
    (chain(minimizer(force2D=1, sensorStdDev="0.1", anything="at all")), (DOF_3, 0, 1.0, 1.0, 0)),
]

# (document, words the refusal holds)
REFUSALS = [
    (chain(minimizer(force2D=1), knn=2), ("PointToPlaneErrorMinimizer", "force2D", "KDTreeMatcher knn >= 2")),
    (chain(minimizer(force4DOF=1), knn=3), ("PointToPlaneErrorMinimizer", "force4DOF", "KDTreeMatcher knn >= 2")),
    (chain(minimizer(force2D=1), outliers=TRIM + ROBUST), ("PointToPlaneErrorMinimizer", "force2D", "RobustOutlierFilter")),
    (chain(minimizer(force4DOF=1), outliers=TRIM + SNO, reading=SN_RD), ("PointToPlaneErrorMinimizer", "force4DOF", "SurfaceNormalOutlierFilter")),
    (chain(minimizer("PointToPlaneWithCovErrorMinimizer", force2D=1)), ("PointToPlaneWithCovErrorMinimizer", "unknown parameter force2D")),
    (chain(minimizer("PointToPlaneWithCovErrorMinimizer", force4DOF=0)), ("PointToPlaneWithCovErrorMinimizer", "unknown parameter force4DOF")),
    (chain(minimizer("PointToPointErrorMinimizer", force2D=1), reference=""), ("PointToPointErrorMinimizer", "force2D")),
    (chain(minimizer("PointToPointErrorMinimizer", force4DOF=0), reference=""), ("PointToPointErrorMinimizer", "force4DOF")),
    (chain(minimizer(force2D=1, force4DOF=1)), ("PointToPlaneErrorMinimizer", "force2D", "force4DOF")),
    (chain(minimizer(force2D=2)), ("PointToPlaneErrorMinimizer", "force2D must be 0 or 1")),
    (chain(minimizer(force4DOF="0.5")), ("PointToPlaneErrorMinimizer", "force4DOF must be 0 or 1")),
    (chain(minimizer(force2D=-1)), ("PointToPlaneErrorMinimizer", "force2D must be 0 or 1")),
    (chain(minimizer(force4DOF="yes")), ("PointToPlaneErrorMinimizer", "force4DOF is not a number")),
    (chain(checkers=COUNTER + bound("-0.1")), ("BoundTransformationChecker", "maxRotationNorm")),
    (chain(checkers=COUNTER + bound("inf")), ("BoundTransformationChecker", "maxRotationNorm")),
    (chain(checkers=COUNTER + bound(trans=".inf")), ("BoundTransformationChecker", "maxTranslationNorm")),
    (chain(checkers=COUNTER + bound(trans="1e39")), ("BoundTransformationChecker", "maxTranslationNorm")),      # infinite as a float
    (chain(checkers=COUNTER + bound(trans="nan")), ("BoundTransformationChecker", "maxTranslationNorm")),
    (chain(checkers=bound() + COUNTER + bound("0.5")), ("BoundTransformationChecker", "given twice")),
    (chain(checkers=COUNTER + "  - BoundTransformationChecker:\n      maxNorm: 1\n"), ("BoundTransformationChecker", "unknown parameter maxNorm")),
    (chain(checkers=bound()), ("CounterTransformationChecker is required",)),
]


def _load(text):
    doc = yaml.load(text, Loader=yaml.BaseLoader) or {}
    return icp.chain_load(doc), icp.chain_load_motion(doc)


def _fields(m):
    return (m.dof, m.bound, m.max_rotation_norm, m.max_translation_norm, m.bound_before_counter)


@pytest.fixture(scope="module")
def cpp_lines(tmp_path_factory):
    """tests/cpp/motion_loader_check.cpp over ACCEPTED and REFUSALS -> ([(facade line, shim line)], its LAYOUT line)"""
    tmp = tmp_path_factory.mktemp("motion_loader")
    exe, docs = str(tmp / "motion_loader_check"), str(tmp / "docs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"), "-I", os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "cpp", "motion_loader_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    texts = [d for d, _ in ACCEPTED] + [d for d, _ in REFUSALS]
    with open(docs, "wb") as f:
        for t in texts:
            b = t.encode()
            f.write(b"DOC %d\n" % len(b) + b)
    r = subprocess.run([exe, docs], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "motion_loader_check: ok %d" % len(texts), r.stdout[-2000:] + r.stderr
    assert lines[-2].startswith("LAYOUT ") and len(lines) == 2 * len(texts) + 2
    return list(zip(lines[0:-2:2], lines[1:-2:2])), lines[-2]


def test_documents_with_the_modules_load_through_the_three_front_ends(cpp_lines):
    """Fails without the feature: on the commit before, BoundTransformationChecker is refused as "not implemented on the HIP
    path", and no front end reports force2D / force4DOF (the parameters load and are ignored)."""
    for (text, want), (line, shim) in zip(ACCEPTED, cpp_lines[0]):
        (rc, why, lc), (rc2, why2, m) = _load(text)
        assert rc == rc2 == _lib.OK, (text, why, why2)
        assert _fields(m) == (want[0], want[1], float(F(want[2])), float(F(want[3])), want[4]), (text, _fields(m))
        assert tuple(m.reserved) == (0, 0, 0)
        o = icp.ICP()
        o.load_from_yaml(io.StringIO(text))
        got = o.chain.motion
        assert got == icp.MotionConfig(want[0], bool(want[1]), float(str(F(want[2]))), float(str(F(want[3]))), bool(want[4])), (text, got)
        # the C++ facade: the same fields, the same bytes of lsgpu_loaded_chain; the shim loads it too
        if want[1]:
            head = "OK %d 1 %.9g %.9g %d " % (want[0], float(F(want[2])), float(F(want[3])), want[4])
        else:
            head = "OK %d 0 - - 0 " % want[0]
        assert line == head + bytes(lc).hex(), text
        assert shim == "SHIM OK", (text, shim)
    assert icp.ICP().chain.motion is None


def test_a_parameter_of_0_and_an_absent_one_load_to_identical_structs():
    base = _load(chain())
    for text in (chain(minimizer(force2D=0)), chain(minimizer(force4DOF=0)), chain(minimizer(force2D=0, force4DOF=0))):
        (rc, why, lc), (rc2, why2, m) = _load(text)
        assert rc == rc2 == _lib.OK, why
        assert bytes(lc) == bytes(base[0][2]) and bytes(m) == bytes(base[1][2])
    m = base[1][2]
    d = _lib.MotionCfg()
    _lib.lib().lsgpu_motion_config_default(C.byref(d))
    assert bytes(m) == bytes(d) and _fields(m) == (0, 0, 1.0, 1.0, 0)
    # the two modules leave lsgpu_loaded_chain as it is: they travel by their own entry
    with_m = _load(chain(minimizer(force2D=1), checkers=bound("0.5", "2") + COUNTER + DIFF))
    assert with_m[0][0] == _lib.OK and bytes(with_m[0][2]) == bytes(base[0][2])


def test_refusals_name_the_module_through_the_three_front_ends(cpp_lines):
    lines = cpp_lines[0][len(ACCEPTED):]
    for (text, words), (line, shim) in zip(REFUSALS, lines):
        (rc, why, _lc), (rc2, why2, _m) = _load(text)
        assert rc == rc2 == _lib.BAD_CONFIG and why == why2, (text, why, why2)
        for w in words:
            assert w in why, (text, why)
        with pytest.raises(_lib.LsgpuError) as e:
            icp.ICP().load_from_yaml(io.StringIO(text))
        assert e.value.code == _lib.BAD_CONFIG and why in str(e.value)
        assert line == "ERR " + why, (text, line)
        assert shim.startswith("SHIM ERR ") and why in shim, (text, shim)


def test_documents_of_the_loader_corpus_carry_neither_module():
    """Every accepted document of tests/golden/chain_loader_corpus.json (none names the two modules or the parameters) loads to
    the default lsgpu_motion_config, every refused one is refused by lsgpu_chain_load_motion with the same text."""
    with open(os.path.join(ROOT, "tests", "golden", "chain_loader_corpus.json")) as f:
        raw = json.load(f)
    docs = ["".join(raw["lines"][i] for i in r["doc"]) for r in raw["entries"]]
    d = _lib.MotionCfg()
    _lib.lib().lsgpu_motion_config_default(C.byref(d))
    n_ok = 0
    for text in docs:
        (rc, why, _lc), (rc2, why2, m) = _load(text)
        assert rc == rc2 and why == why2, (text, why, why2)
        if rc == _lib.OK:
            assert bytes(m) == bytes(d), text
            n_ok += 1
    assert n_ok > 100 and len(docs) - n_ok > 100


# ------------------------------------------------------------------------------------------------ CPU: the ABI

def test_struct_layout_symbols_and_abi_version(cpp_lines):
    L = _lib.lib()
    S = _lib.MotionCfg
    layout = [int(x) for x in cpp_lines[1].split()[1:]]
    assert layout == [C.sizeof(S), S.dof.offset, S.bound.offset, S.max_rotation_norm.offset, S.max_translation_norm.offset,
                      S.bound_before_counter.offset, S.reserved.offset] == [32, 0, 4, 8, 12, 16, 20]
    assert L.lsgpu_abi_version() == 4
    with open(os.path.join(ROOT, "include", "lsgpu_icp.h")) as f:
        header = f.read()
    assert "#define LSGPU_ABI_VERSION 4\n" in header
    names = set(re.findall(r"\b(lsgpu_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    new = {"lsgpu_motion_config_default", "lsgpu_motion_config_check", "lsgpu_motion_config_why", "lsgpu_icp_set_motion",
           "lsgpu_point_to_plane_solve_dof", "lsgpu_bound_first_violation", "lsgpu_chain_load_motion"}
    assert new <= names and new <= set(_lib.ABI_SYMBOLS)
    for name in sorted(names):
        assert hasattr(L, name), name
    for m in re.findall(r"#define (LSGPU_MOTION_DOF_\d) (\d)", header):
        assert getattr(_lib, m[0][len("LSGPU_"):]) == int(m[1])
    c = S()
    c.dof, c.bound, c.max_rotation_norm, c.reserved[1] = 4, 1, 7.0, 9
    L.lsgpu_motion_config_default(C.byref(c))
    assert _fields(c) == (0, 0, 1.0, 1.0, 0) and tuple(c.reserved) == (0, 0, 0)
    assert L.lsgpu_motion_config_check(C.byref(c)) == _lib.OK and L.lsgpu_motion_config_why(C.byref(c)) is None
    for dof, bnd, r, t, before, ok in ((3, 0, 1, 1, 0, True), (4, 1, 0.0, 0.0, 1, True), (0, 1, 3.0, 50.0, 0, True), (3, 0, np.nan, -1, 0, True),
                                       (6, 0, 1, 1, 0, False), (1, 0, 1, 1, 0, False), (-3, 0, 1, 1, 0, False), (0, 2, 1, 1, 0, False),
                                       (0, 1, -0.1, 1, 0, False), (0, 1, 1, np.inf, 0, False), (0, 1, np.nan, 1, 0, False), (0, 1, 1, 1, 2, False)):
        c.dof, c.bound, c.max_rotation_norm, c.max_translation_norm, c.bound_before_counter = dof, bnd, r, t, before
        assert (L.lsgpu_motion_config_check(C.byref(c)) == _lib.OK) == ok, (dof, bnd, r, t, before)
        why = L.lsgpu_motion_config_why(C.byref(c))
        assert (why is None) == ok and (ok or b"PointToPlaneErrorMinimizer" in why or b"BoundTransformationChecker" in why)
    L.lsgpu_motion_config_default(C.byref(c))
    c.reserved[2] = 1
    assert L.lsgpu_motion_config_check(C.byref(c)) == _lib.BAD_CONFIG and L.lsgpu_motion_config_check(None) == _lib.BAD_CONFIG


def test_the_host_entries_as_a_stand_alone_program(tmp_path):
    """tests/cpp/motion_host_check.cpp linked against the library: the loader entry and the two host functions from C++.  (The
    same source builds with -DMOTION_HOST_STANDALONE against the two host-only translation units, for a sanitizer run.)"""
    exe = str(tmp_path / "motion_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "motion_host_check.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("motion_host_check: ok"), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ CPU: the host twins

def random_pairs(seed, n=600, offset=(0.12, -0.07, 0.03), yaw=0.01):
    """n pairs around a box-like scene: points up to 20 m out, unit normals, matches = the points moved back by a small planar
    motion plus 2 cm of noise"""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(-20, 20, (n, 3)) * [1, 1, 0.15]).astype(F)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    c, s = np.cos(yaw), np.sin(yaw)
    q = p.astype(np.float64) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]).T + offset + rng.normal(0, 0.02, (n, 3))
    return p, q.astype(F), nrm


@pytest.mark.parametrize("dof", [DOF_3, DOF_4])
def test_host_twin_equals_the_float64_restatement(dof):
    """Tolerance: the float LLT against a float64 solve of the same system, as tests/test_oracle.py::
    test_point_to_plane_matches_numpy_lstsq holds the 6-DOF float solve (rtol 2e-3, atol 2e-5) -- the solve that
    tests/test_robust_outlier_filter.py::test_point_to_plane_solve_is_the_oracle_step shows lsgpu_point_to_plane_solve to be,
    bit for bit.  Here on the entries of dT: the translation is x[3:6] itself, the rotation's are sin / cos of x[2]."""
    for seed in range(8):
        p, q, nrm = random_pairs(seed)
        s, used = mc.pair_sums(p, q, nrm, dof)
        assert used == 600
        dT = icp.point_to_plane_solve_dof(s, dof)
        assert dT.dtype == F
        x64, dT64 = mc.np_step(s, dof)
        assert abs(x64[2]) > 1e-3 and np.abs(x64[3:5]).min() > 1e-3          # (a step worth the name)
        assert np.allclose(dT.astype(np.float64), dT64, rtol=2e-3, atol=2e-5), (seed, dT, dT64)
        # the fixed unknowns and the third row and column of the rotation: exactly
        assert np.array_equal(bits(dT[2, :3]), bits([0, 0, 1])) and np.array_equal(bits(dT[:3, 2]), bits([0, 0, 1]))
        assert np.array_equal(bits(dT[3]), bits([0, 0, 0, 1]))
        if dof == DOF_3:
            assert bits(dT[2, 3]) == bits(0.0)
        else:
            assert dT[2, 3] != 0
        assert dT[0, 0] == dT[1, 1] and dT[0, 1] == -dT[1, 0]
        # force2D's b differs from the 6-DOF b (the planar residual), A does not
        s6, _ = mc.pair_sums(p, q, nrm, DOF_6)
        assert np.array_equal(s[:21], s6[:21]) and (np.array_equal(s[21:], s6[21:]) == (dof == DOF_4))


def test_host_twin_dof_0_is_the_free_step_bit_for_bit():
    for seed in range(4):
        p, q, nrm = random_pairs(seed)
        s, _ = mc.pair_sums(p, q, nrm, DOF_6)
        assert icp.point_to_plane_solve_dof(s, DOF_6).tobytes() == icp.point_to_plane_solve(s).tobytes()
    with pytest.raises(_lib.ConvergenceError):
        icp.point_to_plane_solve_dof(np.zeros(27), DOF_6)


def test_host_twin_a_yaw_of_zero_is_the_identity_rotation():
    A = np.diag([1.0, 2, 4, 4, 16, 4])                   # (pivots with exact square roots: the quotients are exact scalings)
    dT = icp.point_to_plane_solve_dof(mc.pack(A, [9, 9, 0, 0.4, -1.6, 0.4]), DOF_4)
    assert np.array_equal(bits(dT[:3, :3]), bits(np.eye(3))) and np.array_equal(bits(dT[:3, 3]), bits([0.1, -0.1, 0.1]))
    dT = icp.point_to_plane_solve_dof(mc.pack(A, [9, 9, -0.4, 0.4, -1.6, 0.4]), DOF_3)       # a negative yaw; tz is not solved
    assert dT[1, 0] < 0 and dT[0, 1] == -dT[1, 0] and bits(dT[2, 3]) == bits(0.0)
    assert bits(dT[1, 0]) == bits(-np.sin(np.float64(F(0.1)))) and bits(dT[0, 0]) == bits(np.cos(np.float64(F(0.1))))


def test_host_twin_a_singular_sub_system_is_no_convergence():
    p, q, nrm = random_pairs(0)
    nrm[:] = F([0, 0, 1])                                # every normal along z: yaw, tx and ty are not observed
    for dof in (DOF_3, DOF_4):
        s, _ = mc.pair_sums(p, q, nrm, dof)
        out = np.full(16, np.nan, F)
        rc = _lib.lib().lsgpu_point_to_plane_solve_dof(s.ctypes.data_as(C.POINTER(C.c_double)), dof, icp._fp(out))
        assert rc == _lib.NO_CONVERGENCE and np.array_equal(out.reshape(4, 4), np.eye(4, dtype=F))
        with pytest.raises(_lib.ConvergenceError):
            icp.point_to_plane_solve_dof(s, dof)
    # a sub-system that is fine inside a 6x6 system that is not: roll and pitch unobserved
    A = np.diag([0.0, 0, 3, 4, 5, 6])
    assert icp.point_to_plane_solve_dof(mc.pack(A, np.ones(6)), DOF_4)[0, 3] == F(0.25)
    with pytest.raises(_lib.ConvergenceError):
        icp.point_to_plane_solve(mc.pack(A, np.ones(6)))
    with pytest.raises(_lib.LsgpuError) as e:
        icp.point_to_plane_solve_dof(mc.pack(A, np.ones(6)), 5)
    assert e.value.code == _lib.BAD_ARG


def test_bound_first_violation():
    I = np.eye(4)
    # rotation only (about an axis off z), translation only
    Ts = [I, synth.se3(yaw=0.05, pitch=0.02), synth.se3(yaw=0.2, roll=0.1), synth.se3(yaw=0.01)]
    assert icp.bound_first_violation(Ts, 0.1, 0.0) == mc.np_bound_first_violation(Ts, 0.1, 0.0) == 2
    assert icp.bound_first_violation(Ts, 0.01, 0.0) == 1 and icp.bound_first_violation(Ts, 0.5, 0.0) == -1
    Ts = [I, synth.se3(0.03, 0.04, 0.0), synth.se3(0.3, -0.4, 1.2), synth.se3(0.0, 0.0, 0.01)]
    assert icp.bound_first_violation(Ts, 0.0, 0.1) == mc.np_bound_first_violation(Ts, 0.0, 0.1) == 2
    assert icp.bound_first_violation(Ts, 0.0, 0.01) == 1 and icp.bound_first_violation(Ts, 0.0, 2.0) == -1
    # exactly at the limit is inside (upstream compares with >): |(3, 4, 0)| is 5 in float, one float step below the limit is out
    Ts = [I, synth.se3(3.0, 4.0, 0.0)]
    assert icp.bound_first_violation(Ts, 0.0, 5.0) == -1 and icp.bound_first_violation(Ts, 0.0, float(np.nextafter(F(5), F(0)))) == 1
    # the rotation at its limit: the limit is the checker's own float value of the angle (lsgpu_rotation_distance, the same function)
    Ts = [I, synth.se3(yaw=0.25)]
    ang = F(icp.rotation_distance(Ts[1], Ts[0]))
    assert abs(float(ang) - 0.25) < 1e-6
    assert icp.bound_first_violation(Ts, float(ang), 0.0) == -1 and icp.bound_first_violation(Ts, float(np.nextafter(ang, F(0))), 0.0) == 1
    # out and back in: the first index out
    Ts = [I, synth.se3(0.05), synth.se3(0.5), synth.se3(0.05), synth.se3(0.6)]
    assert icp.bound_first_violation(Ts, 1.0, 0.1) == 2
    # relative to entry 0, not to the identity
    Ts = [synth.se3(10.0, yaw=1.0), synth.se3(10.05, yaw=1.01), synth.se3(10.5, yaw=1.0)]
    assert icp.bound_first_violation(Ts, 0.1, 0.1) == 2 and icp.bound_first_violation(Ts[:2], 0.1, 0.1) == -1
    # n == 1 and n == 0: nothing to compare
    assert icp.bound_first_violation([I], 0.0, 0.0) == -1 and icp.bound_first_violation([], 0.0, 0.0) == -1
    # a NaN entry is not a violation (the loop's own checker reports it)
    bad = I.copy()
    bad[0, 3] = np.nan
    assert icp.bound_first_violation([I, bad, synth.se3(0.5)], 1.0, 0.1) == 2


# ------------------------------------------------------------------------------------------------ GPU

CHAINS = {   # the chain of a handle (IcpHandle's keywords) and the same chain for mc.rebuild_record
    "trimmed": (dict(), dict(trim=0.75)),
    "max_dist_median": (dict(matcher_max_dist=2.0, outlier_median_factor=3.0), dict(trim=0.75, matcher=2.0, median=3.0)),
}


def make_handle(max_iterations=None, **kw):
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))                   # trim 0.75, 40 iterations, differential checker 0.001 / 0.01 / 4
    if max_iterations is not None:
        cfg.max_iterations = max_iterations
    return icp.IcpHandle(cfg, **kw)


@pytest.fixture(scope="module")
def filtered4k(pair4k):
    """the 4 k pair with its reference filtered on the host (SamplingSurfaceNormalDataPointsFilter knn 10, ratio 0.5)"""
    rf, rn = icp.sampling_surface_normal(pair4k["ref"], 10, 0.5, 4)
    return dict(pair4k, rf=np.ascontiguousarray(rf), rn=np.ascontiguousarray(rn))


class _Prims:
    """mc.rebuild_record's primitives on a plain handle with the (centred) search done by the library's kernel-level entries"""
    def __init__(self, h):
        self.h = h
        self.transform_points = h.transform_points
        self.trim_limit = h.trim_limit

    def knn(self, pts):
        return self.h.knn(pts, None)


def _state(T, st, tr):
    return (np.ascontiguousarray(T).tobytes(), int(st.iterations), int(st.converged), F(st.final_limit).tobytes(), int(st.final_n_used),
            mc.trace_bytes(tr))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 4096, 20000])
def test_sums_of_a_constrained_handle(n, pair64k):
    """lsgpu_normal_eq on a force2D handle against the float64 restatement from the ids lsgpu_knn returns: one partial block,
    whole blocks, many blocks.  Tolerance: tests/test_gpu_parity.py::test_normal_eq_matches_oracle's for the 6-DOF sums (relative
    Frobenius / 2-norm error 1e-12 for A, 1e-10 for b).  A force4DOF handle returns the 6-DOF handle's sums bit for bit."""
    rd = np.ascontiguousarray(pair64k["rd"][:n])
    assert len(rd) == n
    with make_handle() as h6, make_handle(motion=dict(dof=DOF_3)) as h3, make_handle(motion=dict(dof=DOF_4)) as h4:
        rf, rn = h6.filter_reference(pair64k["ref"], 10, 0.5, seed=4)
        rf, rn = np.ascontiguousarray(rf), np.ascontiguousarray(rn)
        for h in (h6, h3, h4):
            h.set_reference(rf, rn)
        mean = h6.reference_mean()
        ref_c = rf.copy()
        ref_c[:, :3] -= mean
        T = synth.colmajor(pair64k["T_init"]).copy()
        T[12:15] -= mean
        ids, d2 = h6.knn(rd, T)
        limit = h6.trim_limit(d2, 0.75)
        p = h6.transform_points(T, rd)
        w = d2 <= F(limit)
        out = {}
        for name, h in (("6", h6), ("2d", h3), ("4dof", h4)):
            A, b, used, r2 = h.normal_eq(rd, T, ids, d2, limit)
            assert used == int(w.sum()) >= n // 2
            out[name] = (A, b, r2)
        for name, dof in (("6", DOF_6), ("2d", DOF_3), ("4dof", DOF_4)):
            s, _ = mc.pair_sums(p[w], ref_c[ids[w]], rn[ids[w]], dof)
            Aw, bw = mc.unpack(s)
            A, b, _r2 = out[name]
            ea, eb = np.linalg.norm(A - Aw) / np.linalg.norm(Aw), np.linalg.norm(b - bw) / np.linalg.norm(bw)
            print("n %d %s: A %.3g b %.3g" % (n, name, ea, eb))
            assert ea < 1e-12 and eb < 1e-10, (n, name, ea, eb)
        assert out["4dof"][0].tobytes() == out["6"][0].tobytes() and out["4dof"][1].tobytes() == out["6"][1].tobytes()
        assert out["4dof"][2] == out["6"][2] == out["2d"][2]                       # slot 28 keeps the three-dimensional residual
        assert out["2d"][0].tobytes() == out["6"][0].tobytes() and out["2d"][1].tobytes() != out["6"][1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("chain_name", sorted(CHAINS))
@pytest.mark.parametrize("dof", [DOF_3, DOF_4])
def test_loop_against_the_host(dof, chain_name, filtered4k):
    """Every trace record of an alignment rebuilt on the host: the step from the record's sums with the host twin (T_iter and
    x bit for bit), and the record's limit, pair count (exactly) and sums (the tolerance of the sums test) from a search at
    the previous record's T_iter."""
    kw, ch = CHAINS[chain_name]
    p = filtered4k
    with make_handle(motion=dict(dof=dof), **kw) as h, make_handle() as hk:
        for x in (h, hk):
            x.set_reference(p["rf"], p["rn"])
        T, st = h.align(p["rd"], p["T_init"])
        tr = h.trace()
        mean = hk.reference_mean()
        assert np.array_equal(bits(mean), bits(h.reference_mean()))
        ref_c = p["rf"].copy()
        ref_c[:, :3] -= mean
        T_rm_in = np.asarray(p["T_init"], F).copy()
        T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
        reading = hk.transform_points(synth.colmajor(T_rm_in), p["rd"])
        assert st.iterations == len(tr) >= 4
        T_prev = np.eye(4, dtype=F)
        for i, t in enumerate(tr):
            s_dev = mc.pack(t["A"], t["b"])
            dT = icp.point_to_plane_solve_dof(s_dev, dof)
            T_host = mc.mul4(dT, T_prev)
            assert np.array_equal(bits(T_host), bits(t["T_iter"].reshape(4, 4).T)), (i, T_host, t["T_iter"])
            # x = {0, 0, yaw, tx, ty, tz}: the translation is dT's, the yaw's sine and cosine (in double, rounded) are dT's
            x = t["x"]
            assert np.array_equal(bits(x[3:6].astype(F)), bits(dT[:3, 3])) and np.array_equal(x[3:6], x[3:6].astype(F).astype(np.float64))
            assert x[2] == np.float64(F(x[2])) and x[2] != 0
            assert bits(dT[1, 0]) == bits(np.sin(x[2])) and bits(dT[0, 0]) == bits(np.cos(x[2])), (i, x[2], dT)
            x64, _ = mc.np_step(s_dev, dof)
            assert np.allclose(x, x64, rtol=2e-3, atol=2e-5), (i, x, x64)      # (the tolerance of the host twin's test)
            limit, used, s_host = mc.rebuild_record(_Prims(hk), reading, ref_c, p["rn"], T_prev, ch, dof)
            assert bits(limit) == bits(t["limit"]) and used == t["n_used"], (i, limit, t["limit"], used, t["n_used"])
            Ah, bh = mc.unpack(s_host)
            ea, eb = np.linalg.norm(t["A"] - Ah) / np.linalg.norm(Ah), np.linalg.norm(t["b"] - bh) / np.linalg.norm(bh)
            assert ea < 1e-12 and eb < 1e-10, (i, ea, eb)
            T_prev = T_host
        Tmean = np.eye(4, dtype=F)
        Tmean[:3, 3] = mean
        assert np.array_equal(bits(T), bits(mc.mul4(Tmean, mc.mul4(T_prev, T_rm_in))))
        assert bits(st.final_limit) == bits(tr[-1]["limit"]) and st.final_n_used == tr[-1]["n_used"]


@pytest.fixture(scope="module")
def planar_pair():
    """a pair whose true motion is planar (0.8 m, 0.05 m, 2 degrees of yaw; no pitch), the guess off by a planar 0.25 m / 1 degree"""
    ref, rd, T_true, _T_init = synth.scan_pair(64, pitch_deg=0.0)
    assert np.array_equal(T_true[2], [0, 0, 1, 0]) and np.array_equal(T_true[:3, 2], [0, 0, 1])
    return ref, rd, T_true, synth.se3(0.2, -0.15, 0.0, yaw=np.deg2rad(1.0)) @ T_true


@pytest.mark.gpu
@pytest.mark.parametrize("param,dof", [("force2D", DOF_3), ("force4DOF", DOF_4)])
def test_the_constrained_degrees_of_freedom_stay_fixed(param, dof, planar_pair):
    """A document with the parameter, through ICP.load_from_yaml and compute.  FAILS ON THE COMMIT BEFORE, where the parameter
    loads and is ignored: x[0] and x[1] of the free step are not 0.

    The planarity of the step between consecutive records S = T_i T_{i-1}^-1, in float64.  Every record is a float32 4x4
    whose entries are sums of four float32 products (hostmath::mul4: 4 multiplications, 3 additions, each rounding by at most
    eps32 / 2 of its result), of terms no larger than M = max(1, |t|) over the records' translations.  An entry of a record
    is therefore within 7 / 2 eps32 M of the exact product, S sees two records, and the float64 arithmetic of the test adds
    nothing at this scale: the third row and column of S's rotation lie within 8 eps32 M of (0, 0, 1), and so does S's z
    translation of 0 under force2D.  (The records' own third rows and columns are exact: products with exact 0 and 1.)"""
    ref, rd, T_true, T_init = planar_pair
    o = icp.ICP()
    o.load_from_yaml(io.StringIO(chain(minimizer(**{param: 1}))))
    o.chain.seed = 4
    T = o.compute(rd, ref, T_init)
    st, tr = o.last_stats, o.handle.trace()
    o.handle.close()
    assert st.iterations == len(tr) >= 4
    Ts = [np.eye(4)] + [t["T_iter"].reshape(4, 4).T.astype(np.float64) for t in tr]
    M = max(1.0, max(np.linalg.norm(Ti[:3, 3]) for Ti in Ts))
    tol = 8 * EPS32 * M
    for i, t in enumerate(tr):
        x = t["x"]
        assert bits(x[0].astype(F)) == bits(0.0) and bits(x[1].astype(F)) == bits(0.0) and x[0] == 0 and x[1] == 0, (i, x)
        if dof == DOF_3:
            assert x[5] == 0 and not np.signbit(x[5]), (i, x)
        else:
            assert x[5] != 0
        S = Ts[i + 1] @ np.linalg.inv(Ts[i])
        dev = max(np.abs(S[2, :3] - [0, 0, 1]).max(), np.abs(S[:3, 2] - [0, 0, 1]).max())
        assert dev <= tol, (i, dev, tol)
        if dof == DOF_3:
            assert abs(S[2, 3]) <= tol, (i, S[2, 3], tol)
        Ti = t["T_iter"].reshape(4, 4).T
        assert np.array_equal(bits(Ti[2, :3]), bits([0, 0, 1])) and np.array_equal(bits(Ti[:3, 2]), bits([0, 0, 1]))
    assert st.converged == 1
    dt, dr = synth.pose_error(T.astype(np.float64), T_true)
    print("%s: %d iterations, |dt| %.3g m, |dr| %.3g rad" % (param, st.iterations, dt, dr))
    # (printed, not asserted: this sparse 4 k pair constrains x weakly, and every step -- the free one as well, in a CPU loop with
    #  the oracle's search -- slides to about 0.20 m / 4.6 mrad from the truth before it settles; that is the pair's, not the steps')
    # the correction itself is planar: T = C T_init with C a rotation about z (through the reference's mean) and, force2D, no z
    Cc = T.astype(np.float64) @ np.linalg.inv(np.asarray(T_init, np.float64))
    assert np.abs(Cc[2, :3] - [0, 0, 1]).max() < 1e-5 and np.abs(Cc[:3, 2] - [0, 0, 1]).max() < 1e-5
    if dof == DOF_3:
        assert abs(Cc[2, 3]) < 1e-4


def _bound(rot, trans, before=False):
    return dict(bound=True, max_rotation_norm=rot, max_translation_norm=trans, bound_before_counter=before)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["translation", "rotation"])
def test_the_bound(which, pair4k):
    """A correction of about 0.5 m (or 0.1 rad): a limit below it makes the call fail with T_out = T_init and the checker's
    message, a limit above it leaves T_out, statistics and trace those of the handle without the module.  Through
    lsgpu_icp_align, lsgpu_icp_compute and lsgpu_icp_align_batch."""
    guess = (0.5, 1.5) if which == "translation" else (0.05, 6.0)
    ref, rd, _T_true, T_init = synth.scan_pair(64, guess_err=guess)
    rf, rn = icp.sampling_surface_normal(ref, 10, 0.5, 4)
    tight = _bound(10.0, 0.1) if which == "translation" else _bound(0.02, 100.0)
    loose = _bound(10.0, 5.0) if which == "translation" else _bound(1.0, 100.0)
    with make_handle() as h0, make_handle(motion=loose) as hl, make_handle(motion=tight) as ht:
        for h in (h0, hl, ht):
            h.set_reference(rf, rn)
        rc0, T0, st0, _ = mc.raw_align(h0, rd, T_init)
        tr0 = h0.trace()
        assert rc0 == _lib.OK and st0.iterations >= 4
        # the size of the correction, in the loop's frame
        T_last = tr0[-1]["T_iter"].reshape(4, 4).T
        size = np.linalg.norm(T_last[:3, 3]) if which == "translation" else icp.rotation_distance(T_last, np.eye(4))
        assert (0.3 < size < 0.8) if which == "translation" else (0.06 < size < 0.2), size
        rcl, Tl, stl, errl = mc.raw_align(hl, rd, T_init)
        assert rcl == _lib.OK and errl == "" and _state(Tl, stl, hl.trace()) == _state(T0, st0, tr0)
        rct, Tt, stt, errt = mc.raw_align(ht, rd, T_init)
        assert rct == _lib.NO_CONVERGENCE and np.array_equal(bits(Tt), bits(np.asarray(T_init, F)))
        m = re.fullmatch(r"BoundTransformationChecker: limit out of bounds: rot (\S+)/(\S+) tr (\S+)/(\S+)", errt)
        assert m, errt
        rot, rot_lim, tr, tr_lim = (float(g) for g in m.groups())
        assert (rot_lim, tr_lim) == ((10.0, 0.1) if which == "translation" else (0.02, 100.0))
        assert (tr > tr_lim) if which == "translation" else (rot > rot_lim)
        # ... the first entry out of bounds: what lsgpu_bound_first_violation finds in the records of the unbounded run
        Ts = [np.eye(4)] + [t["T_iter"].reshape(4, 4).T for t in tr0]
        k = icp.bound_first_violation(Ts, tight["max_rotation_norm"], tight["max_translation_norm"])
        assert 1 <= k < len(Ts)
        want = np.linalg.norm(Ts[k][:3, 3].astype(F)) if which == "translation" else icp.rotation_distance(Ts[k], Ts[0])
        assert abs((tr if which == "translation" else rot) - want) <= 1e-5 * want
        with pytest.raises(_lib.ConvergenceError) as e:                # the facade raises what it raises for any ConvergenceError
            ht.align(rd, T_init)
        assert "BoundTransformationChecker" in str(e.value)
        # the module can be taken off and put on again
        ht.set_motion(None)
        assert _state(*ht.align(rd, T_init), ht.trace()) == _state(T0, st0, tr0)
        ht.set_motion(tight)
        # lsgpu_icp_compute (the filters draw: same seed, same clouds)
        Tc0, stc0 = h0.compute(rd, ref, T_init, 0.75, 10, 0.5, seed=4)
        trc0 = h0.trace()
        Tcl, stcl = hl.compute(rd, ref, T_init, 0.75, 10, 0.5, seed=4)
        assert _state(Tcl, stcl, hl.trace()) == _state(Tc0, stc0, trc0)
        with pytest.raises(_lib.ConvergenceError) as e:
            ht.compute(rd, ref, T_init, 0.75, 10, 0.5, seed=4)
        assert "BoundTransformationChecker: limit out of bounds" in str(e.value)
        # lsgpu_icp_align_batch: two pairs per pool
        Tb, stb, rcb = icp.align_batch([hl], [rf, rf], [rn, rn], [rd, rd], [T_init, T_init])
        assert list(rcb) == [_lib.OK, _lib.OK] and all(np.array_equal(bits(Tb[i]), bits(T0)) for i in range(2))
        assert all(stb[i].iterations == st0.iterations for i in range(2))
        Tb, stb, rcb = icp.align_batch([ht], [rf, rf], [rn, rn], [rd, rd], [T_init, T_init])
        assert list(rcb) == [_lib.NO_CONVERGENCE] * 2 and all(np.array_equal(bits(Tb[i]), bits(np.asarray(T_init, F))) for i in range(2))


@pytest.mark.gpu
def test_the_bound_and_the_counters_last_iteration():
    """maxIterationCount 3 on a 0.5 m correction: the counter ends the loop, its last T_iter is in no history.  A limit between
    the first two translations and the third is crossed by that last step only: a checker listed in front of the counter sees
    it, one listed behind does not."""
    ref, rd, _T_true, T_init = synth.scan_pair(64, guess_err=(0.5, 1.5))
    rf, rn = icp.sampling_surface_normal(ref, 10, 0.5, 4)
    with make_handle(3) as h0:
        h0.set_reference(rf, rn)
        rc0, T0, st0, _ = mc.raw_align(h0, rd, T_init)
        tr0 = h0.trace()
    assert rc0 == _lib.OK and st0.iterations == 3 and st0.converged == 0 and len(tr0) == 3
    t = [float(np.linalg.norm(r["T_iter"].reshape(4, 4).T[:3, 3].astype(np.float64))) for r in tr0]
    assert t[2] > 1.02 * max(t[0], t[1]), t                           # the steps of a 0.5 m correction still grow the translation
    lim = 0.5 * (max(t[0], t[1]) + t[2])
    Ts = [np.eye(4)] + [r["T_iter"].reshape(4, 4).T for r in tr0]
    assert icp.bound_first_violation(Ts, 10.0, lim) == 3 and icp.bound_first_violation(Ts[:3], 10.0, lim) == -1
    with make_handle(3, motion=_bound(10.0, lim, before=False)) as hb, make_handle(3, motion=_bound(10.0, lim, before=True)) as hf:
        for h in (hb, hf):
            h.set_reference(rf, rn)
        rc, T, st, err = mc.raw_align(hb, rd, T_init)
        assert rc == _lib.OK and err == "" and _state(T, st, hb.trace()) == _state(T0, st0, tr0)
        rc, T, st, err = mc.raw_align(hf, rd, T_init)
        assert rc == _lib.NO_CONVERGENCE and np.array_equal(bits(T), bits(np.asarray(T_init, F)))
        assert err.startswith("BoundTransformationChecker: limit out of bounds: rot ") and (" tr %.3g" % t[2])[:7] in err, err
        # a limit the first step crosses: found in the history whatever the order
        hb.set_motion(_bound(10.0, 0.5 * t[0], before=False))
        rc, T, st, err = mc.raw_align(hb, rd, T_init)
        assert rc == _lib.NO_CONVERGENCE and "BoundTransformationChecker" in err


@pytest.mark.gpu
def test_a_handle_that_had_the_modules_is_what_it_was(filtered4k):
    p = filtered4k
    with make_handle() as h0, make_handle() as h:
        for x in (h0, h):
            x.set_reference(p["rf"], p["rn"])
        T0, st0 = h0.align(p["rd"], p["T_init"])
        want = _state(T0, st0, h0.trace())
        h.set_motion(dict(dof=DOF_3, **_bound(0.001, 0.001, True)))
        assert h.motion == icp.MotionConfig(DOF_3, True, float(str(F(0.001))), float(str(F(0.001))), True)
        with pytest.raises(_lib.ConvergenceError):
            h.align(p["rd"], p["T_init"])
        h.set_motion(None)
        assert h.motion is None
        assert _state(*h.align(p["rd"], p["T_init"]), h.trace()) == want
        h.set_motion(dict(dof=DOF_4))
        h.set_motion(dict())                                           # the free step, no bound: off as well
        assert h.motion is None
        assert _state(*h.align(p["rd"], p["T_init"]), h.trace()) == want
        A6 = h0.normal_eq(p["rd"], None, *h0.knn(p["rd"], None), 1.0)
        assert all(np.array_equal(a, b) for a, b in zip(h.normal_eq(p["rd"], None, *h.knn(p["rd"], None), 1.0), A6))


@pytest.mark.gpu
def test_refusals_on_the_handle_in_either_order():
    """A GPU test because lsgpu_icp_create opens the device: without one there is no handle to refuse anything."""
    uid = icp.comm_unique_id()
    for dof, word in ((DOF_3, "force2D"), (DOF_4, "force4DOF")):
        m = dict(dof=dof)
        # the other module first, then the constrained step
        for kw, other in ((dict(matcher_knn=2), "KDTreeMatcher knn >= 2"), (dict(robust=dict(robust_fct="cauchy")), "RobustOutlierFilter"),
                          (dict(normals=dict(max_angle=0.6, reading_normals_given=1)), "SurfaceNormalOutlierFilter"),
                          (dict(covariance=0.01), "PointToPlaneWithCovErrorMinimizer"),
                          (dict(error_minimizer="PointToPointErrorMinimizer"), "PointToPointErrorMinimizer")):
            with make_handle(**kw) as h:
                with pytest.raises(_lib.LsgpuError) as e:
                    h.set_motion(m)
                assert e.value.code == _lib.BAD_CONFIG and word in str(e.value) and other in str(e.value) and "PointToPlaneErrorMinimizer" in str(e.value)
                assert h.motion is None
                h.set_motion(_bound(1.0, 1.0))                         # the bound alone goes with all of them
        # the constrained step first, then the other module: refused, the handle keeps what it had
        with make_handle(motion=m) as h:
            for call, other in ((lambda: h.set_robust_filter(dict(robust_fct="cauchy")), "RobustOutlierFilter"),
                                (lambda: h.set_normals(dict(max_angle=0.6, reading_normals_given=1)), "SurfaceNormalOutlierFilter"),
                                (lambda: h.set_covariance(0.01), "PointToPlaneWithCovErrorMinimizer"),
                                (lambda: h.comm_init(0, 1, uid), "split-scan")):
                with pytest.raises(_lib.LsgpuError) as e:
                    call()
                assert e.value.code == _lib.BAD_CONFIG and other in str(e.value) and "force2D / force4DOF" in str(e.value), str(e.value)
            assert h.motion.dof == dof
            for bad in (dict(dof=5), dict(dof=dof, **_bound(-1.0, 1.0)), dict(dof=dof, **_bound(1.0, float("inf")))):
                with pytest.raises(_lib.LsgpuError) as e:
                    h.set_motion(bad)
                assert e.value.code == _lib.BAD_CONFIG
            assert h.motion.dof == dof and not h.motion.bound
    # the split-scan mode and the two modules, either order
    with make_handle(motion=_bound(1.0, 1.0)) as h:
        with pytest.raises(_lib.LsgpuError) as e:
            h.comm_init(0, 1, uid)
        assert e.value.code == _lib.BAD_CONFIG and "BoundTransformationChecker" in str(e.value)
    with make_handle() as h:
        h.comm_init(0, 1, uid)
        for m, word in ((dict(dof=DOF_3), "force2D"), (dict(dof=DOF_4), "force4DOF"), (_bound(1.0, 1.0), "BoundTransformationChecker")):
            with pytest.raises(_lib.LsgpuError) as e:
                h.set_motion(m)
            assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value) and word in str(e.value)
        assert h.motion is None


# ------------------------------------------------------------------------------------------------ CPU: the dump for upstream

def test_the_upstream_dump_carries_the_modules(tmp_path):
    """devtools/dump_for_upstream.py on a chain with force2D and the bound: icp.yaml is the document, the README names the choices."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_for_upstream", os.path.join(ROOT, "devtools", "dump_for_upstream.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    doc = tmp_path / "chain.yaml"
    doc.write_text(chain(minimizer(force2D=1), checkers=bound("0.5", "2") + COUNTER + DIFF))
    rc, iterations = tool.dump(str(tmp_path / "dump"), 64, str(doc))
    assert rc == 0 and iterations > 0
    assert (tmp_path / "dump" / "icp.yaml").read_text() == doc.read_text()
    readme = (tmp_path / "dump" / "README.txt").read_text()
    assert "45 force2D / force4DOF" in readme and "48 BoundTransformationChecker" in readme
    doc.write_text(chain())
    tool.dump(str(tmp_path / "plain"), 64, str(doc))
    assert "force2D" not in (tmp_path / "plain" / "README.txt").read_text()
