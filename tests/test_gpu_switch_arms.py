"""Every arm of tests/switch_arms.py on the GPU: the switches csrc/ reads (the emulator half: tests/test_hostsim_switch_arms.py) with real
MFMA layouts, 256 compute units and real concurrency, and the switches ops.py, models.py and losses.py read, which exist only here.  One
child process per arm (tests/switch_arm_child.py), one at a time, each under its own time limit; the default arm runs through the same
child, so every witness is compared between two fresh processes, neither of them this one.

A child that dies -- a signal, an abort, a segmentation fault, its time limit, HIP's illegal-memory-access error -- ends the module: every
later arm fails at once and starts nothing on the device."""
import subprocess

import pytest

import switch_arms as sa
from test_hostsim_switch_arms import check_arm, run_child

pytestmark = pytest.mark.gpu

# MEASURED on an MI355X: the default arm's child -- it answers every arm's queries: fifteen dispatch cases, three training steps at batch 4,
# two profiler sessions -- takes 6.8-7.1 s from start to exit (1.7 s of them until the library is loaded); an arm's child 2.1-8.3 s, the longest
# being the model arms with their two oracle steps.  The limit is three times the default child's time: it ends a hang, nothing else.
TIMEOUT = 20
DIED = []              # the first arm whose child died
SECONDS = {}


def _child(name, geoms=None):
    if DIED:
        pytest.fail(f"an earlier arm's child died: {DIED[0]}")
    try:
        r, out = run_child(name, "cuda", TIMEOUT, geoms)
    except subprocess.TimeoutExpired:
        DIED.append(name)
        pytest.fail(f"{name}: the child ran into its time limit of {TIMEOUT} s")
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137) or "illegal memory access" in r.stderr:
        DIED.append(name)
        pytest.fail(f"{name}: the child died ({r.returncode}):\n{r.stderr[-3000:]}")
    assert r.returncode == 0 and out is not None, f"{name}: the child failed ({r.returncode}):\n{r.stderr[-3000:]}"
    SECONDS[name] = out["seconds"]
    return out


@pytest.fixture(scope="module")
def default_line():
    out = _child("default")
    yield out
    print("\n[switch arms] seconds per child:", {k: round(v, 1) for k, v in SECONDS.items()}, "total", round(sum(SECONDS.values()), 1))


@pytest.mark.parametrize("name", [n for n in sa.ARMS if n != "default"])
def test_arm_is_reached_and_computes_the_same(default_line, name):
    out = _child(name, default_line["geoms"])
    check_arm(name, "cuda", out, default_line)
