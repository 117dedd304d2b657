"""The gradient guard on the MI355X: hifihr_grad_norm / hifihr_adam_step_guarded through the C ABI on the cases of
tests/test_hostsim_grad_guard.py (tests/grad_guard_cases.py), and the Python surface end to end: FusedAdam(max_grad_norm=...) eager and
captured, and one GraphedTrainStep.  Non-finite values go into the gradient buffer in front of the optimizer step only, never into a batch."""
import pytest
import torch

import grad_guard_cases as gg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from hifihr_amd._lib import get_lib
    assert torch.cuda.is_available()
    return get_lib()


@pytest.mark.parametrize("n", gg.NORM_SIZES + [gg.NORM_SIZE_LARGE])
def test_norm_matches_float64_and_repeats_its_bits(lib, n):
    gg.norm_case(lib, "cuda", n)


@pytest.mark.parametrize("n", [1, 1003])
def test_zero_gradient_has_norm_zero_and_coef_one(lib, n):
    gg.zero_case(lib, "cuda", n)


def test_a_huge_finite_gradient_is_clipped_not_skipped(lib):
    gg.huge_case(lib, "cuda")


@pytest.mark.parametrize("where", ["first", "last_float4", "tail"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_element_clears_the_flag(lib, value, where):
    gg.nonfinite_case(lib, "cuda", value, where)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n,wd", [(1003, 0.0), (4096, 0.01)])
def test_clipped_trajectory_matches_torch(lib, n, wd, counted):
    gg.clipped_trajectory_case(lib, "cuda", n, counted, wd)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n", gg.ADAM_SIZES)
def test_max_norm_inf_is_bit_identical_to_the_unguarded_entry(lib, n, counted):
    gg.inf_is_bit_identical_case(lib, "cuda", n, counted)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n,value", [(1003, float("nan")), (4096, float("-inf"))], ids=["1003-nan", "4096-neg_inf"])
def test_a_non_finite_step_is_skipped_and_still_counts(lib, n, value, counted):
    gg.skip_case(lib, "cuda", n, counted, value)


def test_refusals_write_nothing(lib):
    gg.refusal_case(lib, "cuda")


def _small_module(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Linear(53, 11)).cuda()


def _three_gradients(numel):
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(numel, generator=gen) * s for s in (1.0, 1.0, 30.0)]
    grads[1][numel // 3] = float("nan")
    return [g.cuda() for g in grads]


def test_captured_replay_equals_the_eager_guarded_path():
    """FusedAdam(max_grad_norm=...) in graph mode, its step captured with a static gradient buffer: three replays, the second one with a
    NaN in the gradient, against the eager guarded path on the same gradients -- bit for bit, and grad_stats() reads (3, ., 1)."""
    from hifihr_amd.optim import FlatParams, FusedAdam
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())            # never the legacy default stream before a capture
    try:
        max_norm = 100.0                                   # the norms are about 51, NaN and 1 500: no clip, skip, clip
        eager_flat = FlatParams(_small_module())
        graph_flat = FlatParams(_small_module())
        assert torch.equal(eager_flat.flat, graph_flat.flat)
        # (the padding between tensors stays zero: the gradients below are masked to the parameters' own elements)
        mask = torch.zeros_like(eager_flat.flat)
        for p, o in zip(eager_flat.params, eager_flat.offsets):
            mask[o:o + p.numel()] = 1.0
        grads = [g * mask for g in _three_gradients(eager_flat.numel)]
        # the eager path: the same launches (graph mode: step counter and lr in device memory), one at a time, nothing captured
        eager = FusedAdam(eager_flat, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)
        eager.enable_graph_mode()
        stats_e = []
        for g in grads:
            eager_flat.grad.copy_(g)
            eager.prepare_step()
            eager.step()
            stats_e.append(eager.grad_stats())
        opt = FusedAdam(graph_flat, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm)
        opt.enable_graph_mode()
        graph_flat.grad.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        opt.prepare_step()
        with torch.cuda.graph(graph):
            opt.step()
        assert opt.grad_stats()["steps"] == 0              # (a capture launches nothing)
        for i, g in enumerate(grads):
            graph_flat.grad.copy_(g)
            if i:
                opt.prepare_step()
            graph.replay()
            opt.note_step_done()
            s = opt.grad_stats()
            assert (s["norm"] == stats_e[i]["norm"] or i == 1) and s["clip_coef"] == stats_e[i]["clip_coef"] and s["finite"] == stats_e[i]["finite"]
        torch.cuda.synchronize()
        for a, b, name in ((graph_flat.flat, eager_flat.flat, "params"), (opt.exp_avg, eager.exp_avg, "exp_avg"),
                           (opt.exp_avg_sq, eager.exp_avg_sq, "exp_avg_sq")):
            assert torch.equal(a, b), f"captured and eager guarded steps differ in {name}"
        s = opt.grad_stats()
        assert (s["steps"], s["clipped"], s["skipped"]) == (3, 1, 1) and opt.step_count == 3 and eager.step_count == 3, s
        assert stats_e[2]["clip_coef"] < 1.0 and stats_e[0]["clip_coef"] == 1.0 and not stats_e[1]["finite"]
        assert bool(torch.isfinite(graph_flat.flat).all())
    finally:
        torch.cuda.set_stream(prev)


def test_graphed_train_step_reports_the_norm_and_hides_its_warm_up():
    """One GraphedTrainStep (B = 4, ResNet-18, config 2) with max_grad_norm = inf: after a replay grad_stats().norm is the float64 norm
    of the flat gradient buffer, and the warm-up's steps are not in the counters."""
    from test_gpu_e2e import _setup
    from hifihr_amd.losses import LossFunction
    from hifihr_amd.optim import FlatParams, FusedAdam
    from hifihr_amd.traineval import GraphedTrainStep
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(torch.cuda.Stream())
    try:
        tables, args, model, ref, ex, ex_cpu = _setup(4, graded=True)
        flat = FlatParams(model)
        opt = FusedAdam(flat, lr=1e-6, max_grad_norm=float("inf"))
        step = GraphedTrainStep(model, LossFunction(), opt, ex, args, warmup=2)
        torch.cuda.synchronize()
        s = opt.grad_stats()
        assert (s["steps"], s["clipped"], s["skipped"]) == (0, 0, 0) and opt.step_count == 0, s
        step()
        torch.cuda.synchronize()
        s = opt.grad_stats()
        want = float(flat.grad.double().norm())
        print(f"graphed step: norm {s['norm']!r} float64 {want!r}")
        assert want > 0 and abs(s["norm"] - want) <= gg.NORM_RTOL * want, (s, want)
        assert s["finite"] and s["clip_coef"] == 1.0 and (s["steps"], s["clipped"], s["skipped"]) == (1, 0, 0) and opt.step_count == 1, s
    finally:
        torch.cuda.set_stream(prev)
