"""lsgpu_chain_load, the one rule set behind ICP::loadFromYaml (C++) and ICP.load_from_yaml (Python), against what the two
hand-written loaders it replaced did with a corpus of documents.

tests/golden/chain_loader_corpus.json was recorded on the commit before the loaders were merged: every chain document under
tests/golden/, every document the six tests/cpp/*_loader_check.cpp and their Python twins build, the documents on which the
two loaders disagreed, and the spellings .inf / -.inf / .5 / 1e-3 for every kind of numeric parameter.  Per document: each
loader's verdict, the loaded values (floats as the shortest decimal of the float32), and for a refusal the module (or
section) the parent's text named.  Five entries carry "changed": documents both loaders took and the merged loader
refuses because it checks the parameter names of every module (RandomSampling-, SamplingSurfaceNormalDataPointsFilter,
KDTreeMatcher and the two checkers had no such check).  CPU only."""
import ctypes as C
import io
import json
import os
import subprocess

import numpy as np
import pytest
import yaml

from laser_slam_amd import _lib, icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(x):
    return str(np.float32(x))


def values_of(lc):
    """_lib.LoadedChain -> the corpus's dict of values"""
    i, c, r, n = lc.icp, lc.chain, lc.robust, lc.normals
    v = dict(trim_ratio=_f32(i.trim_ratio), max_iterations=i.max_iterations, min_diff_rot=_f32(i.min_diff_rot),
             min_diff_trans=_f32(i.min_diff_trans), smooth_length=i.smooth_length, error_minimizer=i.error_minimizer,
             matcher_knn=i.matcher_knn, matcher_max_dist=_f32(i.matcher_max_dist), outlier_max_dist=_f32(i.outlier_max_dist),
             outlier_min_dist=_f32(i.outlier_min_dist), outlier_median_factor=_f32(i.outlier_median_factor),
             reading_prob=_f32(c.reading_prob), ssn_knn=c.ssn_knn, ssn_ratio=_f32(c.ssn_ratio), sn_knn=c.sn_knn, robust=None, normals=None)
    if lc.has_robust:
        v["robust"] = dict(robust_fct=r.robust_fct, tuning=_f32(r.tuning), scale_estimator=r.scale_estimator,
                           nb_iteration_for_scale=r.nb_iteration_for_scale, distance_type=r.distance_type, approximation=_f32(r.approximation))
    if lc.has_normals:
        v["normals"] = dict(max_angle=_f32(n.max_angle), reading_sn_knn=n.reading_sn_knn, reading_orient=n.reading_orient,
                            reference_orient=n.reference_orient, reading_sensor=[_f32(x) for x in n.reading_sensor],
                            reference_sensor=[_f32(x) for x in n.reference_sensor])
    return v


@pytest.fixture(scope="module")
def corpus():
    """The file keeps each document as indices into a table of lines and the loaded values as what differs from the first
    golden chain's ("base"): -> [{origin, yaml, cpp: {verdict, values}, python: {verdict, values}, module, changed}]"""
    with open(os.path.join(ROOT, "tests", "golden", "chain_loader_corpus.json")) as f:
        raw = json.load(f)
    out = []
    for r in raw["entries"]:
        e = dict(r, yaml="".join(raw["lines"][i] for i in r["doc"]), cpp=dict(verdict=r["cpp"]), python=dict(verdict=r["python"]))
        for side, key in (("cpp", "values"), ("python", "python_values" if "python_values" in r else "values")):
            if r[side] == "accepted":
                e[side]["values"] = dict(raw["base"], **r[key])
        out.append(e)
    return out


@pytest.fixture(scope="module")
def cpp_lines(corpus, tmp_path_factory):
    """tests/cpp/chain_loader_dump.cpp over the corpus: one "OK <hex of lsgpu_loaded_chain>" / "ERR <text>" line per document"""
    tmp = tmp_path_factory.mktemp("chain_loader")
    exe, docs = str(tmp / "chain_loader_dump"), str(tmp / "corpus.docs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "chain_loader_dump.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")])
    with open(docs, "wb") as f:
        for e in corpus:
            b = e["yaml"].encode()
            f.write(b"DOC %d\n" % len(b) + b)
    r = subprocess.run([exe, docs], capture_output=True, text=True, timeout=60)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "chain_loader_dump: ok %d" % len(corpus), r.stdout[-2000:] + r.stderr
    return lines[:-1]


def test_corpus_holds_what_it_should(corpus):
    origins = {e["origin"] for e in corpus}
    for name in ("icp_chain.yaml", "icp_chain_tight.yaml", "upstream_pair4k/icp.yaml", "upstream_submap3/icp.yaml"):
        path = os.path.join(ROOT, "tests", "golden", name)
        assert any(e["yaml"] == open(path).read() for e in corpus), name
    for check in ("chain_loader_check", "knn_loader_check", "robust_loader_check", "normal_outlier_loader_check", "p2p_loader_check",
                  "surface_normal_loader_check"):
        assert "cpp:" + check in origins, check
    assert sum(o.startswith("py:") for o in origins) >= 6 and sum(o.startswith("issue:") for o in origins) >= 10
    assert {o.split(":")[1] for o in origins if o.startswith("spelling:")} == {".inf", "-.inf", ".5", "1e-3"}
    assert len({e["yaml"] for e in corpus}) == len(corpus)


def test_both_facades_load_the_corpus_as_the_parent_did(corpus, cpp_lines):
    assert len(cpp_lines) == len(corpus)
    failures = []
    for e, line in zip(corpus, cpp_lines):
        kind, _, rest = line.partition(" ")
        # the Python facade: its verdict, its text, the struct the library gave it
        rc, why, lc = icp.chain_load(yaml.load(e["yaml"], Loader=yaml.BaseLoader) or {})
        o = icp.ICP()
        try:
            o.load_from_yaml(io.StringIO(e["yaml"]))
            raised = None
        except _lib.LsgpuError as err:
            raised = err
        where = (e["origin"], e["yaml"])
        parent = (e["cpp"]["verdict"], e["python"]["verdict"])
        if "changed" in e:        # both loaders took it, the issue asks for a refusal (the reason is in the entry)
            assert parent == ("accepted", "accepted") and "only(...)" in e["changed"]
        if "changed" not in e and parent == ("accepted", "accepted") and e["cpp"]["values"] == e["python"]["values"]:
            if rc != _lib.OK or raised is not None or kind != "OK":
                failures.append(("refused, the parent accepted it", where, why, line))
                continue
            if values_of(lc) != e["cpp"]["values"]:
                failures.append(("other values", where, values_of(lc), e["cpp"]["values"]))
        elif "changed" in e or "refused" in parent:
            if rc != _lib.BAD_CONFIG or raised is None or raised.code != _lib.BAD_CONFIG or kind != "ERR":
                failures.append(("accepted, the parent refused it", where, parent, line))
                continue
            if e["module"] not in why or e["module"] not in str(raised) or e["module"] not in rest:
                failures.append(("the text does not name " + e["module"], where, why, rest))
        else:
            failures.append(("both accepted with different values: not a case the corpus should hold unresolved", where))
        # the two facades: the same verdict, the same text, the same bytes
        if rc == _lib.OK:
            if kind != "OK" or bytes.fromhex(rest) != bytes(lc):
                failures.append(("the facades differ", where, line, bytes(lc).hex()))
            elif icp._chain_config(lc) != o.chain:
                failures.append(("ICP.chain is not the loaded chain", where))
        elif kind != "ERR" or rest != why or why not in str(raised):
            failures.append(("the facades differ", where, line, why))
    assert not failures, "%d of %d documents:\n" % (len(failures), len(corpus)) + "\n".join(repr(f) for f in failures[:10])


def test_documents_both_parent_loaders_took_differently_are_resolved(corpus):
    """None in the corpus today: where both accepted, they loaded the same values (`KDTreeMatcher: knn: 2.5`, which the
    Python loader cut to 2, the C++ loader refused)."""
    assert not [e["origin"] for e in corpus if e["cpp"]["verdict"] == e["python"]["verdict"] == "accepted"
                and e["cpp"]["values"] != e["python"]["values"]]


def test_chain_load_directly():
    L = _lib.lib()
    out = _lib.LoadedChain()
    why = C.create_string_buffer(256)
    assert L.lsgpu_chain_load(None, 0, C.byref(out), why, len(why)) == _lib.BAD_CONFIG
    assert why.value == b"matcher: KDTreeMatcher is required"
    assert L.lsgpu_chain_load(None, 0, C.byref(out), None, 0) == _lib.BAD_CONFIG             # a NULL why
    assert L.lsgpu_chain_load(None, 0, C.byref(out), None, 64) == _lib.BAD_CONFIG
    small = C.create_string_buffer(b"\xff" * 16, 16)                                      # too small: cut and NUL-terminated
    assert L.lsgpu_chain_load(None, 0, C.byref(out), small, 12) == _lib.BAD_CONFIG
    assert small.raw[:12] == b"matcher: KD\0" and small.raw[12:] == b"\xff" * 4
    # a refusal leaves *out as it was; an acceptance writes every byte
    mods = [("referenceDataPointsFilters", "SurfaceNormalDataPointsFilter", {"knn": "6"}), ("matcher", "KDTreeMatcher", {"maxDist": ".5"}),
            ("errorMinimizer", "PointToPlaneErrorMinimizer", {}), ("transformationCheckers", "CounterTransformationChecker", {})]

    def call(mods, out):
        arr = (_lib.YamlModule * len(mods))()
        keep = []
        for a, (sec, name, params) in zip(arr, mods):
            ps = (_lib.YamlParam * max(len(params), 1))(*[_lib.YamlParam(k.encode(), v.encode()) for k, v in params.items()])
            keep.append(ps)
            a.section, a.name, a.params, a.n_params = sec.encode(), name.encode(), ps, len(params)
        return L.lsgpu_chain_load(arr, len(mods), C.byref(out), why, len(why))
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    assert call(mods[:3], out) == _lib.BAD_CONFIG and b"CounterTransformationChecker" in why.value
    assert bytes(out) == b"\xab" * C.sizeof(out)
    assert call(mods, out) == _lib.OK and why.value == b""
    assert (out.chain.sn_knn, out.chain.ssn_knn, out.icp.matcher_max_dist, out.icp.max_iterations, out.icp.trim_ratio) == (6, 0, 0.5, 40, 1.0)
    assert out.chain.reading_prob < 0 and out.chain.seed == -1 and (out.has_robust, out.has_normals) == (0, 0) and list(out.reserved) == [0] * 6
    assert C.sizeof(_lib.LoadedChain) == 200 and C.sizeof(_lib.YamlModule) == 32 and C.sizeof(_lib.YamlParam) == 16
    assert L.lsgpu_chain_load(None, 1, C.byref(out), why, len(why)) == _lib.BAD_ARG
    assert L.lsgpu_chain_load(None, 0, None, why, len(why)) == _lib.BAD_ARG


def test_config_why_gives_the_reason_of_the_check():
    L = _lib.lib()
    rb = _lib.RobustCfg()
    L.lsgpu_robust_config_default(C.byref(rb))
    assert L.lsgpu_robust_config_why(C.byref(rb), 0, 1) is None
    rb.tuning = -1.0
    assert L.lsgpu_robust_config_check(C.byref(rb), 0, 1) == _lib.BAD_CONFIG
    assert L.lsgpu_robust_config_why(C.byref(rb), 0, 1) == b"RobustOutlierFilter: tuning must be >= 0"
    nc = _lib.NormalsCfg()
    L.lsgpu_normals_config_default(C.byref(nc))
    assert L.lsgpu_normals_config_why(C.byref(nc), 0, 0) is None
    nc.max_angle = 4.0
    assert L.lsgpu_normals_config_check(C.byref(nc), 0, 1) == _lib.BAD_CONFIG
    assert L.lsgpu_normals_config_why(C.byref(nc), 0, 1) == b"SurfaceNormalOutlierFilter: maxAngle must be in [0, 3.1416]"
    assert L.lsgpu_robust_config_why(None, 0, 1) and L.lsgpu_normals_config_why(None, 0, 1)
