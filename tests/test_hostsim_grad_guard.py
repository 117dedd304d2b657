"""The gradient guard (hifihr_grad_norm / hifihr_adam_step_guarded, csrc/adam.hip) on the hostsim emulator: the shared cases of
tests/grad_guard_cases.py on device='cpu'.  tests/test_gpu_grad_guard.py runs the same bodies on the MI355X."""
import pytest

import grad_guard_cases as gg
import kernel_cases as kc


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.mark.parametrize("n", gg.NORM_SIZES)
def test_norm_matches_float64_and_repeats_its_bits(hostsim_lib, n):
    gg.norm_case(hostsim_lib, "cpu", n)


@pytest.mark.parametrize("n", [1, 1003])
def test_zero_gradient_has_norm_zero_and_coef_one(hostsim_lib, n):
    gg.zero_case(hostsim_lib, "cpu", n)


def test_a_huge_finite_gradient_is_clipped_not_skipped(hostsim_lib):
    gg.huge_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("where", ["first", "last_float4", "tail"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_element_clears_the_flag(hostsim_lib, value, where):
    gg.nonfinite_case(hostsim_lib, "cpu", value, where)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n,wd", [(1003, 0.0), (4096, 0.01)])
def test_clipped_trajectory_matches_torch(hostsim_lib, n, wd, counted):
    gg.clipped_trajectory_case(hostsim_lib, "cpu", n, counted, wd)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n", gg.ADAM_SIZES)
def test_max_norm_inf_is_bit_identical_to_the_unguarded_entry(hostsim_lib, n, counted):
    gg.inf_is_bit_identical_case(hostsim_lib, "cpu", n, counted)


@pytest.mark.parametrize("counted", [False, True], ids=["host_scalars", "counted"])
@pytest.mark.parametrize("n,value", [(1003, float("nan")), (4096, float("-inf"))], ids=["1003-nan", "4096-neg_inf"])
def test_a_non_finite_step_is_skipped_and_still_counts(hostsim_lib, n, value, counted):
    gg.skip_case(hostsim_lib, "cpu", n, counted, value)


def test_refusals_write_nothing(hostsim_lib):
    gg.refusal_case(hostsim_lib, "cpu")


def test_the_new_kernels_are_the_ones_launched(hostsim_lib):
    import torch
    lib = hostsim_lib
    kc.launch_log(lib)
    n = 1003
    guard, ws = lib.grad_guard_alloc(n, "cpu")
    p, g, m, v = torch.ones(n), torch.ones(n), torch.zeros(n), torch.zeros(n)
    lib.grad_norm(g, 1.0, 1.0, guard, ws)
    lib.adam_step_guarded(p, g, m, v, 1.0, gg.LR, gg.B1, gg.B2, gg.EPS, 0.0, 1, None, guard)
    lib.adam_step_guarded(p, g, m, v, 1.0, 0.0, 0.0, 0.0, gg.EPS, 0.0, 0, lib.adam_state_image(gg.LR, gg.B1, gg.B2, 1), guard)
    assert kc.launch_log(lib) == ["grad_sqsum_kernel", "grad_norm_finish_kernel", "adam_kernel_guarded", "adam_kernel_counted_guarded"]
