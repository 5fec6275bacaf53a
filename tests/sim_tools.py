"""The host twin of the step-wise program kinds (tools/prog_sim.cpp) for the *_check modules: one binary, built once per test
session whichever module asks first, and the network prefix that all of its input formats start with."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np

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


# What an engine plans with that a bare Network (prog_sim without options) does not: engine.hip mibn_create / mibn_set_network set
# order_effort 1, second_above and minfill_above from plan_policy.h (base_second_above, base_minfill), and flatten's hints.
ENGINE_PLANNING = dict(order_effort=1, second_above=2e7, minfill_above=5e6)
SIM_OPTIONS = ("small_cells", "big_iters", "tile_h", "order_effort", "second_above", "minfill_above")


def sim_args(f, tmp_path, options=None, ties=False):
    """The option part of a prog_sim command line.  options None: nothing (a bare Network, as every caller before the step matrix
    ran it).  A dictionary: its small_cells / big_iters / tile_h (the engine's set_option values of the same names) on top of what
    an engine plans with - ENGINE_PLANNING and the network's hints -, so that the twin's program is the engine's word for word."""
    args = ["--ties"] if ties else []
    if options is None:
        return args
    unknown = set(options) - set(SIM_OPTIONS)
    assert not unknown, unknown
    for k, v in {**ENGINE_PLANNING, **options}.items():
        args += [f"--{k}", repr(v) if isinstance(v, float) else str(int(v))]
    path = os.path.join(str(tmp_path), "hints.txt")
    with open(path, "w") as fh:
        fh.write(f"{len(f.hints)}\n" + "\n".join(" ".join(map(str, np.asarray(h).tolist())) for h in f.hints) + "\n")
    return args + ["--hints", path]


def parse_ties(stderr):
    """[(request, cells with tied maxima, those a traceback read)] from the lines prog_sim --ties leaves on standard error."""
    return [tuple(int(x) for x in line.split()[1:4]) for line in stderr.splitlines() if line.startswith("ties ")]


def network_prefix(f):
    """The lines every input of prog_sim starts with: n_vars, card, scope_off, scope_vars, value_off, values (hex floats)."""
    return [str(len(f.card)), " ".join(map(str, f.card)), " ".join(map(str, f.scope_off)), " ".join(map(str, f.scope_vars)),
            " ".join(map(str, f.value_off)), " ".join(float(x).hex() for x in f.values)]
