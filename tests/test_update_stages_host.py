"""The staged per-iteration update against the serial one, on the CPU (tests/cpp/update_stages_check.cpp): both are
compiled for the host from csrc/lsgpu_solve.hip.h, the staged form is run "for each stage, for each thread index", and the
loop state, the checker history and the trace records must agree byte for byte -- for every minimizer, with and without
the robust filter's part, over every exit of the update.  Built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staged_update_matches_the_serial_update_on_the_host(tmp_path):
    exe = str(tmp_path / "update_stages_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "update_stages_check.cpp"), "-o", exe])
    # the first 6x6 system of the 4 k golden pair: 36 doubles A, 6 doubles b, the inlier count, the limit
    z = np.load(os.path.join(ROOT, "tests", "golden", "icp_pair4k.npz"))
    system = str(tmp_path / "golden_system.bin")
    np.concatenate([z["A0"].ravel(), z["b0"].ravel(), [float(z["used0"])], [float(z["limit0"])]]).astype(np.float64).tofile(system)
    r = subprocess.run([exe, system], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "UPDATE_STAGES_OK" in r.stdout and "golden system included" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
