"""The self-supervised keypoint terms (csrc/losses.hip: hifihr_open2d_terms_fwd / _bwd) and the launch that feeds them (csrc/augment.hip:
hifihr_freihand_keypoints) on the host emulator.  The cases are those of tests/test_gpu_open2d.py (tests/open2d_cases.py); the reference is
the float64 restatement of tests/open2d_ref.py."""
import pytest

import kernel_cases as kc
import open2d_cases as oc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.mark.parametrize("case", oc.TERM_CASES, ids=_ids)
def test_terms_match_the_float64_restatement(hostsim_lib, case):
    oc.terms_case(hostsim_lib, "cpu", *case)


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    oc.refusal_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("case", oc.KEYPOINT_CASES, ids=_ids)
def test_keypoint_launch_matches_the_restatement(hostsim_lib, case):
    oc.keypoints_case(hostsim_lib, "cpu", *case)


def test_keypoint_launch_takes_flat_confidences(hostsim_lib):
    oc.keypoints_case(hostsim_lib, "cpu", 3, "random", 0.5, con3=False)


def test_keypoint_refusals_and_indices_outside_the_cache(hostsim_lib):
    oc.keypoints_refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    oc.terms_case(hostsim_lib, "cpu", *oc.TERM_CASES[1])
    oc.keypoints_case(hostsim_lib, "cpu", 3, "zero", None)
    log = set(kc.launch_log(hostsim_lib))
    assert oc.KERNELS | {"freihand_keypoints_kernel"} <= log, log
