"""The adaptive planning policy and the device planner's share rule (sorobn_amd/csrc/plan_policy.h) on the host: tools/plan_policy_sim.cpp
includes the header the engine includes, is fed scripted sequences and prints the state after every command.  The expected values are worked
out here from the rules as the header's comments state them and from its three constants - none is copied from the program's output."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "sorobn_amd", "csrc", "plan_policy.h")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _constant(name):
    return float(re.search(r"#define %s ([0-9.]+)" % name, open(HEADER).read()).group(1))


KEEPS_UP, WINDOW_MS, BOUND = (_constant(n) for n in ("MIBN_HOST_KEEPS_UP", "MIBN_POLICY_WINDOW_MS", "MIBN_HOST_BOUND_RATIO"))
BASE_MINFILL = 5e6


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "plan_policy_sim")
    r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "plan_policy_sim.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*lines):
        """-> the state after each line of the script, as dicts of floats"""
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        states = [{k: float(v) for k, v in (kv.split("=") for kv in ln.split())} for ln in out.stdout.splitlines()]
        assert len(states) == len(lines)
        return states
    return run


def _warm(threads, nets="1 1"):
    """adaptive on; calls 1 and 2 with nothing measured yet (the marks stay at zero)"""
    return ["set adaptive 1", f"start 1 {threads} 0 0 0 {nets}", f"start 2 {threads} 0 0 0 {nets}"]


def test_constants_are_the_documented_ones():
    assert (KEEPS_UP, WINDOW_MS, BOUND) == (1.25, 150.0, 1.15)


def test_seeding_starts_a_starved_rank_on_the_device_planner(sim):
    s = sim("set adaptive 1", "start 1 2 0 0 0 1 1")[-1]
    assert (s["gpu_emit"], s["auto_emit"], s["seeded"]) == (1, 1, 1)
    s = sim("set adaptive 1", "start 1 16 0 0 0 1 1")[-1]  # a full rank: seeded, nothing switched
    assert (s["gpu_emit"], s["auto_emit"], s["seeded"]) == (0, 0, 1)
    s = sim("start 1 2 0 0 0 1 1")[-1]  # the policy is off
    assert (s["gpu_emit"], s["seeded"]) == (0, 0)


def test_first_two_calls_only_advance_the_marks(sim):
    a, b = sim("set adaptive 1", "start 1 16 400 100 1000 1 1", "start 2 16 900 200 2000 1 1")[1:]
    assert (a["seen_plan_ms"], a["seen_kernel_ms"], a["seen_requests"]) == (400, 100, 1000)
    assert (b["seen_plan_ms"], b["seen_kernel_ms"], b["seen_requests"]) == (900, 200, 2000)
    for s in (a, b):  # (400 against 100 ms would be host-bound, were it judged)
        assert (s["streak"], s["gpu_emit"], s["kernel_ms_per_req"]) == (0, 0, 0)


def test_a_small_window_is_neither_judged_nor_consumed(sim):
    assert 100 < WINDOW_MS
    a, b = sim(*_warm(16), "start 3 16 100 100 1000 1 1", "start 4 16 300 260 2000 1 1")[-2:]
    assert (a["seen_plan_ms"], a["seen_kernel_ms"], a["seen_requests"], a["streak"], a["kernel_ms_per_req"]) == (0, 0, 0, 0, 0)
    # the next call sees the accumulated window: 300 ms of planning against 260 of kernels over 2 000 requests
    assert 300 > BOUND * 260
    assert (b["seen_plan_ms"], b["seen_kernel_ms"], b["seen_requests"], b["streak"]) == (300, 260, 2000, 1)
    assert b["kernel_ms_per_req"] == pytest.approx(260 / 2000, rel=1e-15)
    # a starved rank judges what a full rank does not: 100 against 80 ms
    c = sim(*_warm(4, "0 0"), "start 3 4 100 80 1000 0 0")[-1]
    assert 100 > BOUND * 80 and (c["streak"], c["seen_plan_ms"]) == (1, 100)


def test_host_bound_twice_in_a_row_switches_the_device_planner_on(sim):
    assert 200 / 160 > BOUND >= 160 / 160
    s = sim(*_warm(16), "set host_rate 3.0",
            "start 3 16 200 160 1000 1 1",   # host-bound: the streak only
            "start 4 16 360 320 2000 1 1",   # (160, 160): resets it
            "start 5 16 560 480 3000 1 1",   # host-bound again: 1
            "start 6 16 760 640 4000 1 1")   # twice in a row
    assert [(x["streak"], x["gpu_emit"], x["auto_emit"]) for x in s[-4:]] == [(1, 0, 0), (0, 0, 0), (1, 0, 0), (2, 1, 1)]
    assert s[-2]["host_rate"] == 3.0 and s[-1]["host_rate"] == 0  # measured afresh beside the device planner
    assert s[-1]["gpu_search"] == 0 and s[-1]["minfill_above"] == BASE_MINFILL
    # a network with an order net but no emit net gets the device order search instead
    t = sim(*_warm(16, "1 0"), "start 3 16 200 160 1000 1 0", "start 4 16 400 320 2000 1 0")[-1]
    assert (t["gpu_emit"], t["gpu_search"], t["auto_search"]) == (0, 1, 1)


def test_the_device_planner_is_given_back_where_the_host_alone_keeps_up(sim):
    setup = ["set auto_emit 1", "set gpu_emit 1", "set host_rate 2.0"]
    assert 2.0 * 0.7 >= KEEPS_UP > 2.0 * 0.6
    s = sim(*_warm(16), *setup, "start 3 16 200 700 1000 1 1")[-1]  # 0.7 ms of kernels per request
    assert (s["gpu_emit"], s["auto_emit"], s["streak"]) == (0, 0, 0)
    s = sim(*_warm(16), *setup, "start 3 16 200 600 1000 1 1")[-1]  # 0.6: it stays
    assert (s["gpu_emit"], s["auto_emit"]) == (1, 1) and s["kernel_ms_per_req"] == pytest.approx(0.6, rel=1e-15)


def test_without_an_order_net_the_minfill_bar_moves(sim):
    s = sim(*_warm(4, "0 0"), "start 3 4 200 160 1000 0 0", "start 4 4 400 320 2000 0 0",  # host-bound twice: x 8
            "start 5 4 440 520 3000 0 0",                                                    # 40 < 0.3 x 200: back
            "set minfill_above %r" % (2 * BASE_MINFILL), "start 6 4 480 720 4000 0 0")      # ... never below the base
    assert 40 < 0.3 * 200
    assert [x["minfill_above"] for x in (s[3], s[4], s[5], s[7])] == [BASE_MINFILL, 8 * BASE_MINFILL, BASE_MINFILL, BASE_MINFILL]
    assert all(x["gpu_emit"] == 0 and x["gpu_search"] == 0 for x in s)


def test_share_follows_the_two_rates_latency_bound_rule(sim):
    # the host's 8 192 requests took 8 ms: in the device's 8 ms it plans 8 192 of 32 768 - the device's share 0.75
    s = sim("set emit_share 0.75", "chunk 32768 24576 8 8 32768 0")[-1]
    assert s["emit_share"] == 0.75 and s["host_rate"] == 1024 and s["ruled"] == 0
    # in 16 ms it plans 16 384: 0.5, averaged with the share so far
    s = sim("set emit_share 0.75", "chunk 32768 24576 8 16 32768 0")[-1]
    assert s["emit_share"] == 0.5 * 0.75 + 0.5 * 0.5 == 0.625
    # the rate is smoothed by halves
    s = sim("set host_rate 512", "chunk 32768 24576 8 8 32768 0")[-1]
    assert s["host_rate"] == 0.5 * 512 + 0.5 * 1024


def _wave_target(n, nd, host_ms, dev_ms, host_rate, kv, fixed_per_req):
    ih = max(host_ms / (n - nd), 1.0 / host_rate if host_rate > 0 else 0.0)
    kp = dev_ms / nd
    return max(0.03, min(0.99, (n * ih + fixed_per_req * n - 0.85 * kv * n) / ((ih + 0.85 * kp) * n)))


def test_share_wave_mode_rule(sim):
    n, nd, host_ms, dev_ms = 32768, 16384, 32.768, 16.384  # the host plans 500 requests per ms, the planner's kernels 1 000
    for kv, fixed, want in ((0.001, 0.0005, None), (0.004, 0.0005, 0.03), (0.004, 0.01, 0.99)):
        s = sim("set emit_share 0.5", "set kernel_ms_per_req %r" % kv, "set fixed_ms_per_req %r" % fixed, f"chunk {n} {nd} {host_ms} {dev_ms} 32768 1")[-1]
        rate = (n - nd) / host_ms
        target = _wave_target(n, nd, host_ms, dev_ms, rate, kv, fixed)
        if want is None:  # by hand: (0.002 + 0.0005 - 0.00085) / (0.002 + 0.00085) = 0.57894...
            assert target == pytest.approx(0.00165 / 0.00285, rel=1e-12) and 0.03 < target < 0.99
        else:
            assert target == want  # clamped
        assert s["ruled"] == 1 and s["host_rate"] == pytest.approx(rate, rel=1e-15)
        assert s["emit_share"] == pytest.approx(0.5 * 0.5 + 0.5 * target, rel=1e-12)
    # the rate in wave mode is smoothed 3 : 1; without retired kernel time the latency-bound rule applies
    s = sim("set host_rate 1000", "set emit_share 0.5", f"chunk {n} {nd} {host_ms} {dev_ms} 32768 1")[-1]
    assert s["host_rate"] == pytest.approx(0.75 * 1000 + 0.25 * 500, rel=1e-15) and s["ruled"] == 0
    assert s["emit_share"] == pytest.approx(0.5 * 0.5 + 0.5 * (1.0 - (n - nd) / host_ms * dev_ms / n), rel=1e-12)


def test_tail_chunks_unmeasurable_times_and_a_pinned_share(sim):
    assert 4 * 20000 < 3 * 32768
    s = sim("set emit_share 0.75", "chunk 20000 15000 5 8 32768 0")[-1]  # the tail of a call: the rate, not the share
    assert (s["host_rate"], s["emit_share"]) == (1000, 0.75)
    s = sim("set emit_share 0.75", "chunk 32768 24576 0.02 8 32768 0")[-1]  # host time too short to measure: neither
    assert (s["host_rate"], s["emit_share"]) == (0, 0.75)
    s = sim("set emit_share 0.5", "set emit_share_opt 0.5", "chunk 32768 16384 8 16 32768 0", "chunk 32768 16384 8 16 32768 1")  # pinned: never moved
    assert [x["emit_share"] for x in s[2:]] == [0.5, 0.5] and s[2]["host_rate"] == 2048


def test_device_share_of_a_chunk(sim):
    nd = lambda *lines: sim(*lines)[-1]["nd"]
    assert nd("set emit_share 0.5", "set emit_share_opt 0.5", "share 512 0 1") == 256  # the host keeps 256: the fewest it is left with
    assert nd("set emit_share 0.75", "share 300 0 1") == 300                            # fewer than 256 left: the device takes the chunk
    assert nd("set emit_share 0.5", "share 512 1 1") == 512                             # gpu_emit = 2: every request
    assert nd("set emit_share 1.0", "share 32768 0 1") == int(32768 * 0.99 + 0.5)       # unpinned: at most 0.99 (wave planner) ...
    assert nd("set emit_share 1.0", "share 32768 0 0") == int(32768 * 0.95 + 0.5)       # ... or 0.95
    assert nd("set emit_share 1.0", "set emit_share_opt 1.0", "share 32768 0 1") == 32768


def test_fixed_cost_per_request_is_smoothed_by_halves(sim):
    a, b = sim("end 1000 20", "end 4000 40")
    assert a["fixed_ms_per_req"] == 0.02 and b["fixed_ms_per_req"] == 0.5 * 0.02 + 0.5 * 0.01
