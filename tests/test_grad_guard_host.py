"""Host logic of the gradient guard (no GPU): which entries FusedAdam.step() calls with the option off and on, which values the option
takes, the guard block's layout, and the option's way through options.py / train_hrnet.py.  The library is a stub that records calls."""
import math
import os
import struct
import sys

import pytest
import torch


class _Stub:
    def __init__(self):
        from hifihr_amd._lib import HifihrLib
        self.calls = []
        self.adam_state_image = HifihrLib.adam_state_image

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def record(*args):
            self.calls.append((name, args))
        return record


class _State:                                            # stands in for the device tensor of the counted state
    def copy_(self, image):
        pass


def _optimizer(monkeypatch, **kw):
    import hifihr_amd.optim as optim
    monkeypatch.setattr(optim, "require_cuda", lambda *t: None)        # (host logic on CPU tensors: the stub launches nothing)
    opt = optim.FusedAdam(optim.FlatParams(torch.nn.Linear(4, 3)), lr=1e-3, grad_scale=0.5, **kw)
    stub = _Stub()
    opt._lib = stub
    return opt, stub


def test_option_off_calls_exactly_the_unguarded_entries(monkeypatch):
    opt, stub = _optimizer(monkeypatch)
    assert opt.max_grad_norm is None and opt._guard is None and opt.grad_stats() is None and opt.guard_snapshot() is None
    opt.step(); opt.step()
    assert [c[0] for c in stub.calls] == ["adam_step", "adam_step"] and stub.calls[1][1][-1] == 2 and opt.step_count == 2
    stub.calls.clear()
    opt.graph_mode, opt._state = True, _State()
    opt.prepare_step(); opt.step()
    assert [c[0] for c in stub.calls] == ["adam_step_counted"] and opt.step_count == 3


@pytest.mark.parametrize("max_norm", [1.0, 5, float("inf")])
def test_option_on_calls_norm_then_the_guarded_entry_in_both_modes(monkeypatch, max_norm):
    opt, stub = _optimizer(monkeypatch, max_grad_norm=max_norm)
    assert opt.max_grad_norm == float(max_norm) and opt._guard.numel() == 32 and opt._guard.dtype == torch.uint8
    assert opt._guard_ws.numel() >= 8 and not opt._guard.any()
    guard, ws = opt._guard, opt._guard_ws
    opt.step()
    names = [c[0] for c in stub.calls]
    assert names == ["grad_norm", "adam_step_guarded"], names
    norm_args, step_args = stub.calls[0][1], stub.calls[1][1]
    assert norm_args[0] is opt.flatp.grad and norm_args[1:3] == (0.5, float(max_norm)) and norm_args[3] is guard and norm_args[4] is ws
    assert step_args[0] is opt.flatp.flat and step_args[1] is opt.flatp.grad and step_args[4] == 0.5        # the SAME grad_scale
    assert step_args[-3] == 1 and step_args[-2] is None and step_args[-1] is guard and opt.step_count == 1
    stub.calls.clear()
    state = _State()
    opt.graph_mode, opt._state = True, state
    opt.prepare_step(); opt.step()
    names = [c[0] for c in stub.calls]
    assert names == ["grad_norm", "adam_step_guarded"], names
    assert stub.calls[1][1][-2] is state and stub.calls[1][1][-1] is guard and opt.step_count == 2
    assert opt._guard is guard and opt._guard_ws is ws            # allocated once: captured graphs hold the addresses
    with pytest.raises(RuntimeError, match="prepare_step"):
        opt.step()                                               # (the eager launch in graph mode still needs its prepare_step)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("-inf"), "1.0", True, [1.0]])
def test_bad_max_grad_norm_values_raise(bad):
    from hifihr_amd.optim import FlatParams, FusedAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(FlatParams(torch.nn.Linear(4, 3)), max_grad_norm=bad)


def test_guard_block_layout_and_snapshot():
    from hifihr_amd._lib import HifihrLib, LIB_PATH
    from hifihr_amd.optim import FlatParams, FusedAdam
    lib = HifihrLib(LIB_PATH)
    assert int(lib.c.hifihr_grad_guard_bytes()) == 32
    sizes = [int(lib.c.hifihr_grad_norm_workspace_bytes(n)) for n in (0, 1, 1024, 1028, 12_000_005)]      # one workgroup per 256 float4
    assert all(s >= 8 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[2] < sizes[3]
    raw = struct.pack("<dfiiiii", 2.5, 0.25, 1, 7, 3, 2, 0)
    assert lib.grad_guard_unpack(raw) == {"norm": 2.5, "clip_coef": 0.25, "finite": True, "steps": 7, "clipped": 3, "skipped": 2}
    opt = FusedAdam(FlatParams(torch.nn.Linear(4, 3)), max_grad_norm=1.0)
    snap = opt.guard_snapshot()
    opt._guard.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    assert opt.grad_stats()["steps"] == 7
    opt.guard_restore(snap)
    assert opt.grad_stats() == {"norm": 0.0, "clip_coef": 0.0, "finite": False, "steps": 0, "clipped": 0, "skipped": 0}
    assert set(opt.state_dict()) == {"step", "exp_avg", "exp_avg_sq", "param_groups"}          # the counters are not persisted


def test_option_reaches_the_training_front_end():
    from hifihr_amd import options
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import train_hrnet as T
    assert options.baseline_config2_args(train_batch=2).max_grad_norm == 0.0
    assert T.build_args(T.parse([])).max_grad_norm == 0.0 and T.optimizer_max_grad_norm(T.build_args(T.parse([]))) is None
    a = T.build_args(T.parse(["--max_grad_norm", "2.5"]))
    assert a.max_grad_norm == 2.5 and T.optimizer_max_grad_norm(a) == 2.5
    a = T.build_args(T.parse(["--max_grad_norm", "inf"]))
    assert math.isinf(a.max_grad_norm) and T.optimizer_max_grad_norm(a) == float("inf")
    line = T.grad_guard_log({"norm": 12.5, "clip_coef": 0.5, "finite": True, "steps": 40, "clipped": 3, "skipped": 1})
    assert line == " gnorm=1.250e+01 clipped=3/40 skipped=1" and T.grad_guard_log(None) == ""
