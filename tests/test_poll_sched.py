"""The poll schedules of the granule gather on the CPU: g++ builds tests/poll_sched_check.cpp from
the header the kernels are built from (bmc_plan.h: PollSched, poll_issue_state).  The first reads
of a spaced schedule must go out at strictly increasing, evenly spaced wait states; a schedule that
is not spaced issues its reads back to back, and every schedule keeps two reads in flight (three
and four were slower, spaced or not: DESIGN 4.1)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WAIT_STATE_CYCLES = 4.3     # one s_nop wait state on MI355X (scripts/micro/pollsched.hip)
LOAD_ROUND_TRIP = 260       # cycles of a dependent sc1 load from L2 (scripts/micro/pingpong.hip)


@pytest.fixture(scope="module")
def schedules(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is required")
    exe = tmp_path_factory.mktemp("poll") / "poll_sched_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                        os.path.join(HERE, "poll_sched_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        name, depth, first, gap, *times = line.split()
        table[name] = (int(depth), int(first), int(gap), [int(t) for t in times])
    return table


def test_every_use_has_a_schedule(schedules):
    assert set(schedules) == {"local", "agent", "plain", "level2"}
    for name, (depth, first, gap, times) in schedules.items():
        assert depth == 2 and len(times) == depth, name
        assert first >= 0 and gap >= 0 and times[0] == first, name


def test_issue_times_increase_evenly(schedules):
    for name, (depth, first, gap, times) in schedules.items():
        steps = {b - a for a, b in zip(times, times[1:])}
        assert steps == {gap}, name                      # evenly spaced
        if gap:
            assert all(b > a for a, b in zip(times, times[1:])), name


def test_the_spaced_pair_samples_within_a_round_trip(schedules):
    """The local pair is spaced, and by less than a load round trip: spaced by a whole one the
    second read would sample when the re-issued first one does."""
    depth, first, gap, times = schedules["local"]
    assert gap > 0
    assert 0.25 * LOAD_ROUND_TRIP < gap * WAIT_STATE_CYCLES < 0.75 * LOAD_ROUND_TRIP
    # what is not spaced is exactly the earlier schedule, apart from the agent scope's first read
    assert schedules["plain"][1:3] == (0, 0) and schedules["level2"][1:3] == (0, 0)
    assert schedules["agent"][2] == 0 and schedules["agent"][1] > 0
