"""The staged per-iteration update of k_normal_eq_loop's last block against the serial icp_update_lane, on the device: the
alignments of tests/update_stages_worker.py in two processes -- the default, and LSGPU_SPLIT_UPDATE=1, under which the
update is the serial function (the stand-alone k_icp_update; for the weighted launches, which must run the update
themselves, lane 0 of the last block).  The staged form changes which lane executes an operation, never the operation, its
operands or their order: the transform, the iteration count and every trace field must be bit-identical."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINIMIZERS = ["point_to_plane", "point_to_point", "force4dof", "force2d"]
SOURCES = ["synth", "golden"]   # the 4 k pair from the generator, and as tests/golden/icp_pair4k.npz holds it
FIELDS = ["limit", "n_used", "A", "b", "x", "T_iter"]


def _run(env_add):
    env = dict(os.environ)
    env.pop("LSGPU_SPLIT_UPDATE", None)
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "update_stages_worker.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("UPDATE_STAGES ")]
    assert r.returncode == 0 and line, (env_add, r.stdout[-1500:], r.stderr[-1500:])
    return json.loads(line[0][len("UPDATE_STAGES "):])


@pytest.fixture(scope="module")
def runs():
    """(staged, serial): every case of the worker, once per process."""
    return _run({}), _run({"LSGPU_SPLIT_UPDATE": "1"})


def _same(runs, case):
    staged, serial = runs[0][case], runs[1][case]
    assert staged["iterations"] == serial["iterations"] and staged["converged"] == serial["converged"], (case, staged["iterations"], serial["iterations"])
    assert staged["n_trace"] == serial["n_trace"] == staged["iterations"], case
    assert staged["T"] == serial["T"], case
    for f in FIELDS:
        for it, (a, b) in enumerate(zip(staged[f], serial[f])):
            assert a == b, (case, f, it)
    assert staged["robust_trace"] == serial["robust_trace"], case
    return staged


@pytest.mark.gpu
@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("minimizer", MINIMIZERS)
def test_staged_update_is_the_serial_update(runs, minimizer, src):
    res = _same(runs, minimizer + "/" + src)
    assert res["iterations"] >= 5, res["iterations"]   # (a chain, not one step)


@pytest.mark.gpu
@pytest.mark.parametrize("src", SOURCES)
def test_staged_update_of_a_robust_chain(runs, src):
    res = _same(runs, "robust/" + src)
    assert res["iterations"] >= 5 and len(res["robust_trace"]) == res["iterations"], res["iterations"]


@pytest.mark.gpu
@pytest.mark.parametrize("src", SOURCES)
def test_staged_update_ends_by_the_counter(runs, src):
    res = _same(runs, "by_counter/" + src)
    assert res["iterations"] == 3 and res["converged"] == 0, res


@pytest.mark.gpu
@pytest.mark.parametrize("src", SOURCES)
def test_staged_update_ends_by_the_differential_checker(runs, src):
    res = _same(runs, "by_differential/" + src)
    assert res["converged"] == 1 and res["iterations"] < 40, res
