"""The off arms of the dispatch switches that csrc/ reads, on the hostsim emulator: tests/switch_arms.py lists them, tests/switch_arm_child.py
runs one per process (the switches are cached in function-local statics: setting a variable inside this process would test the default arm
again).  Each arm must (a) answer its witness queries differently from a default process, both answers as the table writes them, and
(b) pass its cases -- the shared contract bodies at their own bounds, plus hifihr_conv2d_describe against the launch log.  The GPU half:
tests/test_gpu_switch_arms.py."""
import json
import os
import subprocess
import sys

import pytest

import switch_arms as sa

HERE = os.path.dirname(os.path.abspath(__file__))
TIMEOUT = 600          # an arm takes 3-15 s here (8 convolution cases at ~1.4 s); the limit only ends a process that hangs
PLAIN = {"fwd", "fwd_bnstats", "bwd_data", "bwd_weight"}      # entries conv_contract_expect decides, whatever the switches say


def run_child(arm, device, timeout, geoms=None):
    """-> (CompletedProcess, the JSON line or None); every switch of the table is taken out of the environment first"""
    env = {k: v for k, v in os.environ.items() if k not in sa.ALL_SWITCHES}
    env.update(sa.ARMS[arm]["env"])
    cmd = [sys.executable, os.path.join(HERE, "switch_arm_child.py"), arm, device] + ([json.dumps(geoms)] if geoms else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    try:
        return r, (json.loads(lines[-1]) if lines else None)
    except ValueError:
        return r, None


def norm(v):
    return json.loads(json.dumps(v))


def check_arm(name, device, out, default):
    """the witness pair and the cases of one arm's JSON line against the table and the default process's line"""
    arm = sa.ARMS[name]
    ws = sa.witness(arm, device)
    assert ws or arm["unseen"].get(device), f"{name}: no witness on {device} and no reason why"
    assert len(out["witness"]) == len(ws) == len(default["witness"][name])
    for (q, want_default, want_arm), got_default, got_arm in zip(ws, default["witness"][name], out["witness"]):
        assert got_default == norm(want_default), f"{name}: {q} in a default process: {got_default}, the table says {want_default}"
        if want_arm is None:              # a conv_log query: the arm's own log for that case is one of its cases, and differs
            logs = [c[2] for c in sa.cases(arm, device) if c[0] == "dispatch" and c[1] == q[1]]
            assert logs and sorted(map(tuple, logs[0])) != sorted(map(tuple, q[2])), f"{name}: no dispatch case with another log than the default's for {q[1]}"
        else:
            assert got_arm == norm(want_arm), f"{name}: {q} under the arm: {got_arm}, the table says {want_arm}"
    if ws and not any(norm(d) != norm(a) for _, d, a in ws):
        raise AssertionError(f"{name}: no witness query changes under the arm")
    done = out["cases"]
    assert [norm(c["case"]) for c in done] == norm(sa.cases(arm, device)), f"{name}: the child ran other cases than the table lists"
    for c in done:
        # every case the contract documents as accepted is accepted under the arm too (the case bodies assert it per entry; what the
        # arm's own predicates refuse -- the fused entries, a pair -- must come back refused and untouched, which they assert as well)
        if c["case"][0] == "conv":        # `documented`: kernel_cases.conv_contract_expect of the geometry, as the child read it
            assert set(c["accepted"]["documented"]) == PLAIN, (name, c)
            assert {e: c["accepted"][e] for e in PLAIN} == c["accepted"]["documented"], (name, c)
        assert 0.0 <= c["ratio"] <= 1.0, (name, c)
    print(f"\n[switch arm] {name} on {device}: largest err / bound {out['max_ratio']:.3f} over {len(done)} cases, "
          f"{out['seconds']:.1f} s ({out['startup_seconds']:.1f} s to start)")
    assert out["max_ratio"] <= 1.0


CABI = [n for n, a in sa.ARMS.items() if n != "default" and "cpu" in sa.devices(a)]


@pytest.fixture(scope="module")
def default_line():
    r, out = run_child("default", "cpu", TIMEOUT)
    assert r.returncode == 0 and out is not None, f"the default arm's child failed ({r.returncode}):\n{r.stderr[-3000:]}"
    return out


@pytest.mark.parametrize("name", CABI)
def test_arm_is_reached_and_computes_the_same(default_line, name):
    assert len(sa.cases(sa.ARMS[name], "cpu")) <= 8, "at most 8 cases per arm on the emulator"
    r, out = run_child(name, "cpu", TIMEOUT)
    assert r.returncode == 0 and out is not None, f"{name}: the child failed ({r.returncode}):\n{r.stderr[-3000:]}"
    check_arm(name, "cpu", out, default_line)
