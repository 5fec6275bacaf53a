"""The host twin of the step-wise program kinds (tools/prog_sim.cpp) for the *_check modules: one binary, built once per test
session whichever module asks first, and the network prefix that all of its input formats start with."""
import atexit
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_exe = None


def build_prog_sim():
    """-> the path of prog_sim, linked against planner.cpp (-ffp-contract=off: its `draw` computes the device's bits)."""
    global _exe
    if _exe is None:
        d = tempfile.mkdtemp(prefix="prog_sim_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "prog_sim")
        r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "prog_sim.cpp"),
                            os.path.join(ROOT, "sorobn_amd", "csrc", "planner.cpp"), "-lpthread", "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        _exe = exe
    return _exe


def network_prefix(f):
    """The lines every input of prog_sim starts with: n_vars, card, scope_off, scope_vars, value_off, values (hex floats)."""
    return [str(len(f.card)), " ".join(map(str, f.card)), " ".join(map(str, f.scope_off)), " ".join(map(str, f.scope_vars)),
            " ".join(map(str, f.value_off)), " ".join(float(x).hex() for x in f.values)]
