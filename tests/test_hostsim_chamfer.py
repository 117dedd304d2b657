"""The Chamfer distance (csrc/chamfer.hip: hifihr_chamfer_fwd / _bwd) on the host emulator.  The cases are those of
tests/test_gpu_chamfer.py (tests/chamfer_cases.py); the reference is the float64 restatement of tests/chamfer_ref.py, pinned to the
reference's own ChamferLoss by tests/golden/chamfer.npz."""
import os

import pytest

import chamfer_cases as cc
import kernel_cases as kc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


def test_known_answers(hostsim_lib):
    cc.known_answers_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("ni", range(5))
def test_boundaries_match_the_restatement(hostsim_lib, ni):
    """N = the ni-th of {1, Q-1, Q, Q+1, 2Q+3} against every M of {1, T-1, T, T+1, 2T+5}"""
    Ns, Ms = cc.boundary_sizes(hostsim_lib)
    for M in Ms:
        cc.boundary_case(hostsim_lib, "cpu", Ns[ni], M)


def test_ties_go_to_the_lowest_index(hostsim_lib):
    cc.tie_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("N,M", [(778, 778), (5990, 778)])
def test_product_sizes(hostsim_lib, N, M):
    cc.product_case(hostsim_lib, "cpu", 1, N, M)


def test_zero_weights(hostsim_lib):
    cc.zero_weight_case(hostsim_lib, "cpu")


def test_null_gradients(hostsim_lib):
    cc.null_gradient_case(hostsim_lib, "cpu")


def test_reference_chamfer_loss(hostsim_lib):
    cc.golden_case(hostsim_lib, "cpu", GOLDEN)


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    cc.refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    cc.boundary_case(hostsim_lib, "cpu", 3, 5)
    assert cc.KERNELS <= set(kc.launch_log(hostsim_lib))
