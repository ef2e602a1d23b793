"""Which modules a handle runs together (csrc/lsgpu_modules.h): the rule function on the CPU and the library's setters on the GPU,
both against tests/golden/module_rules_parent.json -- what the eight lsgpu_icp_set_* and lsgpu_icp_comm_init answered to
module_cases.drive() before the rule set existed -- and lsgpu_chain_load_modules / lsgpu_icp_set_modules against the part loaders
and the eight setters they stand for, over the documents of tests/golden/chain_loader_corpus.json."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import yaml

from laser_slam_amd import _lib, icp

import module_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "module_rules_parent.json")) as f:
        fx = json.load(f)
    assert fx["variants"] == mc.VARIANTS and fx["configs"] == mc.CONFIGS and fx["texts"][0] == ""
    return fx


def test_rule_function_answers_as_the_setters_did(tmp_path, parent):
    """tests/cpp/modules_check.cpp: every ordered pair of module variants on the four handle configurations, the refused removals,
    lsgpu_icp_comm_init behind every single module, every setter under a communicator -- text for text what the fixture holds."""
    exe = str(tmp_path / "modules_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "modules_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[-2:] == ["modules_check: ok", ""], r.stdout[-2000:] + r.stderr
    texts = parent["texts"]
    n = len(mc.VARIANTS)
    got = {c: dict(pairs=[[None] * n for _ in range(n)], comm_init=[None] * n, removals={}, with_comm=[None] * n) for c in mc.CONFIGS}
    ix = lambda t: -1 if t == "-" else texts.index(t)      # (a text the parent never gave: ValueError names it)
    for ln in lines[:-2]:
        kind, config, *rest = ln.split("\t")
        if kind == "pairs":
            got[config]["pairs"][int(rest[0])][int(rest[1])] = [ix(rest[2]), ix(rest[3])]
        elif kind == "removals":
            got[config]["removals"][rest[0]] = [ix(t) for t in rest[1:]]
        else:
            got[config][kind][int(rest[0])] = ix(rest[1])
    want = {c: dict(parent["setters"][c], with_comm=parent["with_comm"][c]) for c in mc.CONFIGS}
    assert got == want
    # the fixture is not trivially equal: both verdicts, in numbers, and the texts of both directions of a pair
    flat = [v for c in mc.CONFIGS for row in want[c]["pairs"] for pair in row for v in pair]
    assert len(flat) == 4 * n * n * 2 and flat.count(0) > 500 and len(flat) - flat.count(0) > 300 and len(set(flat)) > 25
    assert all(v > 0 for c in mc.CONFIGS for v in want[c]["with_comm"])
    assert all(v != 0 for c in mc.CONFIGS for v in want[c]["comm_init"]) and any(v > 0 for v in want["plane_knn1"]["comm_init"])
    for m, seq in want["plane_knn1"]["removals"].items():
        assert seq[:2] == [0, 0] and seq[2] > 0 and seq[3] > 0 and "remove the module first" in texts[seq[2]], m


@pytest.mark.gpu
def test_setters_answer_as_recorded(parent):
    """The driver that made the fixture, on the library as it is now: one handle per configuration, a few hundred host calls,
    no cloud and no kernel; every reset between two sequences returns LSGPU_OK (module_cases.Handle.reset asserts it)."""
    texts = list(parent["texts"])
    got = mc.encode(mc.drive(mc.Handle), texts)
    assert texts == parent["texts"], texts[len(parent["texts"]):]      # no text the parent did not give
    assert got == parent["setters"]


# ---------------------------------------------------------------------------------- one loader call, one apply call
@pytest.fixture(scope="module")
def corpus():
    """The documents of tests/golden/chain_loader_corpus.json that are YAML mappings (the facades refuse the others themselves)"""
    with open(os.path.join(ROOT, "tests", "golden", "chain_loader_corpus.json")) as f:
        raw = json.load(f)
    docs = []
    for e in raw["entries"]:
        text = "".join(raw["lines"][i] for i in e["doc"])
        try:
            doc = yaml.load(text, Loader=yaml.BaseLoader)
        except Exception:
            continue
        if isinstance(doc, dict):
            docs.append((text, doc))
    return docs


def _old_parts(doc, carried):
    """What the facades loaded before lsgpu_chain_load_modules: (rc, why) of the first loader that refuses, and the five parts"""
    rc, why, lc = icp.chain_load(doc, carried)
    if carried:
        rcp, whyp, cuts, shadow, motion, cs = icp.chain_load_parts_carried(doc, carried)
        assert (rcp, whyp) == (rc, why)
    else:
        (rc1, why1, cuts), (rc2, why2, shadow) = icp.chain_load_cuts(doc), icp.chain_load_shadow(doc)
        (rc3, why3, motion), (rc4, why4, cs) = icp.chain_load_motion(doc), icp.chain_load_cov_sampling(doc)
        assert {(rc, why)} == {(rc1, why1), (rc2, why2), (rc3, why3), (rc4, why4)}
    return rc, why, (lc, cuts, shadow, motion, cs)


def test_one_walk_loads_what_the_part_loaders_load(corpus):
    """lsgpu_chain_load_modules over every document of the corpus, accepted or refused, under every declaration of carried
    normals: the verdict and text of the part loaders, and their bytes part for part."""
    verdicts = set()
    for text, doc in corpus:
        for carried in (0, _lib.CARRIED_READING, _lib.CARRIED_REFERENCE, _lib.CARRIED_READING | _lib.CARRIED_REFERENCE):
            rc, why, parts = _old_parts(doc, carried)
            rcm, whym, m = icp.chain_load_modules(doc, carried)
            assert (rcm, whym) == (rc, why), (carried, text)
            verdicts.add(rc)
            if rc != _lib.OK:
                assert bytes(m) == bytes(_lib.ChainModules())           # (a refusal writes nothing)
                continue
            got = (m.chain, m.cuts, m.shadow, m.motion, m.cov_sampling)
            assert [bytes(g) for g in got] == [bytes(p) for p in parts], (carried, text)
            assert m.carried == carried and list(m.reserved) == [0, 0, 0]
    assert verdicts == {_lib.OK, _lib.BAD_CONFIG} and len(corpus) > 300
    arr, n, _keep = icp._yaml_modules(corpus[0][1])
    assert _lib.lib().lsgpu_chain_load_modules(arr, n, 4, C.byref(_lib.ChainModules()), None, 0) == _lib.BAD_ARG    # an unknown bit
    assert _lib.lib().lsgpu_chain_load_modules(arr, n, 0, None, None, 0) == _lib.BAD_ARG


def _record(doc):
    rc, why, m = icp.chain_load_modules(doc, 0)
    return m if rc == _lib.OK else None


def _eight_setters(h, parts):
    """The facades' ritual before lsgpu_icp_set_modules, on IcpHandle h -> (code, text) of the first setter that refuses, or (OK, "")"""
    lc, cuts, shadow, motion, cs = parts
    sd, md = C.c_float(), C.c_float()
    has_cov = _lib.lib().lsgpu_loaded_chain_covariance(C.byref(lc), C.byref(sd))
    has_md = _lib.lib().lsgpu_loaded_chain_max_density(C.byref(lc), C.byref(md))
    steps = [(lc.has_robust, h.set_robust_filter, lc.robust), (lc.has_normals, h.set_normals, lc.normals),
             (has_cov, h.set_covariance, sd.value), (cuts.n_reading or cuts.n_reference, h.set_chain_cuts, cuts),
             (has_md, h.set_max_density, md.value), (shadow.reading_eps >= 0 or shadow.reference_eps >= 0, h.set_shadow, shadow),
             (cs.reading_nb_sample > 0 or cs.reference_nb_sample > 0, h.set_cov_sampling, cs), (motion.dof or motion.bound, h.set_motion, motion)]
    for present, setter, cfg in steps:
        if present:
            try:
                setter(cfg)
            except _lib.LsgpuError as e:
                return e.code, _lib.lib().lsgpu_last_error(h._h).decode()
    return _lib.OK, ""


def _apply(h, m):
    rc = _lib.lib().lsgpu_icp_set_modules(h._h, C.byref(m))
    return rc, _lib.lib().lsgpu_last_error(h._h).decode()


def _quality(h):
    try:
        return h.quality()
    except _lib.LsgpuError as e:
        return e.code, str(e)


def _module_key(m):
    c = m.chain
    return (c.icp.error_minimizer, c.icp.matcher_knn, bytes(c.robust) if c.has_robust else b"", bytes(c.normals) if c.has_normals else b"",
            bytes(c.reserved), bytes(m.cuts), bytes(m.shadow), bytes(m.motion), bytes(m.cov_sampling))


def _reported(h):
    n = h.normals
    return (bytes(h.robust) if h.robust is not None else None, bytes(n) if n is not None else None, h.covariance,
            bytes(h.cuts) if h.cuts is not None else None, h.max_density, h.shadow, h.cov_sampling, h.motion, h.reads_reference_normals())


@pytest.mark.gpu
def test_one_apply_call_is_the_eight_setters(corpus):
    """Every accepted document: loaded once and applied with lsgpu_icp_set_modules on one handle, loaded part by part and applied
    with the eight setters in the facades' order on a second -- the same code and text, the same answer of lsgpu_icp_get_quality;
    and the handle the Python facade makes of the document (one record from its keyword arguments, one call) reports what the
    handle of the eight set_* methods reports."""
    accepted = 0
    for text, doc in corpus:
        m = _record(doc)
        if m is None:
            continue
        accepted += 1
        _rc, _why, parts = _old_parts(doc, 0)
        facade = icp.ICP()
        facade.load_from_yaml(text)
        if m.chain.icp.max_iterations < 1:                           # (a document the loader takes and lsgpu_icp_create does not)
            for make in (lambda: icp.IcpHandle(m.chain.icp), lambda: facade.handle):
                with pytest.raises(_lib.LsgpuError) as e:
                    make()
                assert e.value.code == _lib.BAD_CONFIG
            continue
        with icp.IcpHandle(m.chain.icp) as ha, icp.IcpHandle(m.chain.icp) as hb:
            assert _apply(ha, m) == _eight_setters(hb, parts) == (_lib.OK, ""), text
            assert _quality(ha) == _quality(hb) and _quality(ha)[0] in (_lib.BAD_CONFIG, _lib.NO_CONVERGENCE), text
            assert _apply(ha, m) == (_lib.OK, "")                    # (the same set again)
            hf = facade.handle
            assert _reported(hf) == _reported(hb), text
            assert _quality(hf) == _quality(hb), text
            facade._handle.close()
    assert accepted > 100


@pytest.mark.gpu
def test_one_apply_call_computes_what_the_eight_setters_compute(corpus):
    """One compute on the 4 k pair per distinct module set among the accepted documents: T and the trace of the handle behind
    lsgpu_icp_set_modules equal, bit for bit, those of the handle behind the eight setters."""
    import chain_cuts_cases
    pair = np.load(os.path.join(ROOT, "tests", "golden", "icp_pair4k.npz"))
    rd, ref, T_init = pair["rd"], pair["ref"], pair["T_init"]
    seen, computed = set(), 0
    for text, doc in corpus:
        m = _record(doc)
        if m is None or m.chain.icp.max_iterations < 1 or _module_key(m) in seen:
            continue
        seen.add(_module_key(m))
        _rc, _why, parts = _old_parts(doc, 0)
        c = m.chain.chain
        out = []
        with icp.IcpHandle(m.chain.icp) as ha, icp.IcpHandle(m.chain.icp) as hb:
            assert _apply(ha, m) == _eight_setters(hb, parts) == (_lib.OK, ""), text
            for h in (ha, hb):
                try:
                    T, st = h.compute(rd, ref, T_init, c.reading_prob, c.ssn_knn, c.ssn_ratio, 11, c.sn_knn)
                    out.append((T.tobytes(), int(st.iterations), chain_cuts_cases.trace_bytes(h), repr(_quality(h))))
                    computed += h is ha
                except _lib.LsgpuError as e:
                    out.append((e.code, str(e)))
        assert out[0] == out[1], text
    assert len(seen) >= 25 and computed >= 20


def _refused_sets():
    """(what it is, handle configuration, the set): sets some step refuses, behind steps that pass"""
    L = _lib.lib()
    def base():
        m = _lib.ChainModules()
        L.lsgpu_shadow_config_default(C.byref(m.shadow))
        L.lsgpu_motion_config_default(C.byref(m.motion))
        L.lsgpu_cov_sampling_config_default(C.byref(m.cov_sampling))
        return m
    def with_normals(m, knn=5):
        m.chain.normals, m.chain.has_normals = mc.variant("normals_angle_knn" if knn else "normals_angle")[1], 1
    def with_cov(m):
        m.chain.reserved[0], m.chain.reserved[1] = 1, int(np.float32(0.01).view(np.int32))
    sets = []
    m = base(); m.chain.robust, m.chain.has_robust = mc.variant("robust")[1], 1; with_cov(m)
    sets.append(("robust, then the covariance", "plane_knn1", m))
    m = base(); with_normals(m); m.shadow.reading_eps = 0.1; m.motion.dof = _lib.MOTION_DOF_3
    sets.append(("reading normals, Shadow on the reading, then force2D", "plane_knn1", m))
    m = base(); m.cov_sampling.reading_nb_sample = 100; m.motion.bound = 1
    sets.append(("CovarianceSampling on the reading without its normals", "plane_knn1", m))
    m = base(); m.cuts = mc.variant("cuts")[1]; with_cov(m); m.chain.reserved[4], m.chain.reserved[5] = 1, int(np.float32(10).view(np.int32))
    sets.append(("cuts and the covariance, then MaxDensity", "plane_knn1", m))
    m = base(); m.cuts = mc.variant("cuts")[1]; m.motion.dof = _lib.MOTION_DOF_4
    sets.append(("cuts, then force4DOF on a point-to-point handle", "point", m))
    m = base(); m.shadow.reference_eps = 0.1; with_cov(m)
    sets.append(("the covariance on a knn 2 handle", "knn2", m))
    m = base(); m.shadow.reference_eps = 5.0
    sets.append(("a value the module's own check refuses", "chain_threshold", m))
    return sets


@pytest.mark.gpu
def test_a_refused_set_leaves_the_handle_as_it_was():
    """lsgpu_icp_set_modules on a set the setters refuse: the code and text of the first setter that refuses, and nothing applied
    -- the steps that passed before it included: the modules of the accepted set that was there stay, and that set applies again."""
    L = _lib.lib()
    texts = set()
    for what, config, m in _refused_sets():
        parts = (m.chain, m.cuts, m.shadow, m.motion, m.cov_sampling)
        with icp.IcpHandle(mc.icp_config(config)) as ha, icp.IcpHandle(mc.icp_config(config)) as hb:
            want = _eight_setters(hb, parts)
            assert want[0] == _lib.BAD_CONFIG and want[1], what
            texts.add(want[1])
            # on an empty handle: refused as the setters refuse, and still empty -- the reading's Shadow finds no normals to stand on
            assert _apply(ha, m) == want, what
            assert L.lsgpu_icp_set_shadow(ha._h, C.byref(mc.variant("shadow_reading")[1])) == _lib.BAD_CONFIG
            assert "(lsgpu_icp_set_normals with reading_sn_knn) first" in L.lsgpu_last_error(ha._h).decode(), what
            assert _quality(ha)[0] == _lib.BAD_CONFIG                 # (the covariance is not on)
            # on a handle with an accepted set (BoundTransformationChecker alone, which every configuration takes): refused alike,
            # and the accepted set applies again
            ok = _lib.ChainModules.from_buffer_copy(_refused_sets()[0][2])
            ok.chain.has_robust, ok.chain.reserved[0] = 0, 0
            ok.motion.bound = 1
            assert _apply(ha, ok) == (_lib.OK, ""), what
            assert _apply(ha, m) == want, what
            assert _apply(ha, ok) == (_lib.OK, ""), what
    assert len(texts) == len(_refused_sets())
    # a step that passes in front of the one that refuses must not stay: normals and the reading's Shadow pass, force2D refuses; had
    # they stayed, removing the normals (the next set's second step) would be refused in front of the step that removes Shadow
    what, config, m = _refused_sets()[1]
    with icp.IcpHandle(mc.icp_config(config)) as h:
        assert _apply(h, m)[0] == _lib.BAD_CONFIG
        empty = _lib.ChainModules.from_buffer_copy(m)
        empty.chain.has_normals, empty.shadow.reading_eps, empty.motion.dof = 0, -1.0, 0
        assert _apply(h, empty) == (_lib.OK, "")
    assert L.lsgpu_icp_set_modules(None, C.byref(m)) == _lib.BAD_ARG
