"""The point-to-mesh distance (csrc/point_mesh.hip: hifihr_point_mesh_fwd / _bwd) on the host emulator.  The cases are those of
tests/test_gpu_point_mesh.py (tests/point_mesh_cases.py); the reference is the float64 restatement of tests/point_mesh_ref.py."""
import pytest

import kernel_cases as kc
import point_mesh_cases as pc


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


def test_known_answers(hostsim_lib):
    pc.known_answers_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("ni", range(5))
def test_boundaries_match_the_restatement(hostsim_lib, direction, ni):
    """The ni-th query count of {1, Q-1, Q, Q+1, 2Q+3} against every searched count of {1, T-1, T, T+1, 2T+5}, for the (Q, T) of the points ->
    faces search (direction 0: Q points, T faces) and of the faces -> points search (direction 1: Q faces, T points)"""
    Ns, Fs = pc.boundary_sizes(hostsim_lib, direction)
    pairs = [(Ns[ni], F) for F in Fs] if direction == 0 else [(N, Fs[ni]) for N in Ns]
    for N, F in pairs:
        pc.boundary_case(hostsim_lib, "cpu", N, F)


def test_ties_go_to_the_lowest_index(hostsim_lib):
    pc.tie_case(hostsim_lib, "cpu")


def test_mano_topology(hostsim_lib):
    pc.mano_case(hostsim_lib, "cpu", 1)


def test_zero_weights(hostsim_lib):
    pc.zero_weight_case(hostsim_lib, "cpu")


def test_null_gradients(hostsim_lib):
    pc.null_gradient_case(hostsim_lib, "cpu")


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    pc.refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    pc.boundary_case(hostsim_lib, "cpu", 3, 5)
    assert pc.KERNELS <= set(kc.launch_log(hostsim_lib))
