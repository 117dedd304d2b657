"""The one-launch keypoint fit (csrc/mano_fit.hip: hifihr_mano_fit) on the host emulator.  The cases are those of
tests/test_gpu_mano_fit.py (tests/mano_fit_cases.py) with iteration counts an emulator can afford; the reference is the float64 restatement
of tests/mano_fit_ref.py."""
import pytest

import kernel_cases as kc
import mano_fit_cases as fc


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.fixture(scope="module")
def tables_of(synth_tables, mano_dense):
    return {"synth": synth_tables, "dense": mano_dense[0]}


@pytest.mark.parametrize("case", fc.EVAL_CASES, ids=lambda c: c[0])
def test_iters_0_matches_float64_autograd(hostsim_lib, tables_of, case):
    fc.eval_case(hostsim_lib, "cpu", tables_of[case[6]], *case[:6])


@pytest.mark.parametrize("iters,with3d", [(1, False), (5, False), (5, True)])
def test_trajectory_matches_the_float64_restatement(hostsim_lib, synth_tables, iters, with3d):
    fc.trajectory_case(hostsim_lib, "cpu", synth_tables, iters, with3d=with3d)


@pytest.mark.parametrize("parts", ["ab", "c", "de"])
def test_invariances(hostsim_lib, synth_tables, parts):
    fc.invariance_case(hostsim_lib, "cpu", synth_tables, iters=2, parts=parts)


def test_a_non_finite_hand_stops_alone(hostsim_lib, synth_tables):
    fc.nonfinite_case(hostsim_lib, "cpu", synth_tables, iters=2)


def test_refusals_leave_the_outputs_untouched(hostsim_lib, synth_tables):
    fc.refusal_case(hostsim_lib, "cpu", synth_tables)


def test_the_fit_is_one_launch(hostsim_lib, synth_tables):
    kc.launch_log(hostsim_lib)
    fc.trajectory_case(hostsim_lib, "cpu", synth_tables, 1)
    log = kc.launch_log(hostsim_lib)
    assert log == [fc.KERNEL], log
