"""The move-only owners of device buffers, pinned buffers, events and streams (sorobn_amd/csrc/device_mem.h) on the host:
tools/device_mem_sim.cpp includes the header the engine includes against a fake HIP runtime (tools/fake_hip) that backs every handle with
malloc and keeps a ledger of creates and releases, and is built with the address and undefined-behaviour sanitizers.  The program asserts:
an empty owner's destructor makes no backend call; ensure() below capacity makes none, above it frees once and allocates once at the
policy sizes (need + need/2 + 1024 elements, bytes + bytes/4 + 4096 pinned); moves, move assignment over a live owner and self move
assignment release every handle exactly once; with a failure injected at each creation in turn, a struct of one of each owner releases
what was created once and nothing twice."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_device_mem_owners(tmp_path):
    exe = str(tmp_path / "device_mem_sim")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "tools", "fake_hip"), os.path.join(ROOT, "tools", "device_mem_sim.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    assert out.stdout.strip() == "device_mem_sim: ok"
