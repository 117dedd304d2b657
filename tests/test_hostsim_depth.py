"""The depth map and the depth loss (csrc/depth.hip: hifihr_render_depth_fwd / _bwd, hifihr_depth_loss_fwd / _bwd) on the host emulator.
The cases are those of tests/test_gpu_depth.py (tests/depth_cases.py); the references are oracle/raster_oracle.c and the restatements of
tests/depth_ref.py."""
import pytest

import depth_cases as dc
import kernel_cases as kc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


def test_known_answers(hostsim_lib):
    dc.known_answers_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("kind", dc.KINDS)
def test_depth_has_the_bits_of_the_rasteriser(hostsim_lib, kind):
    dc.bit_equality_case(hostsim_lib, "cpu", kind)


def test_mano_topology_has_the_bits_of_the_rasteriser(hostsim_lib, synth_tables):
    dc.mano_bits_case(hostsim_lib, "cpu", synth_tables)


@pytest.mark.parametrize("case", dc.GRAD_CASES, ids=_ids)
def test_gradient_matches_float64_autograd(hostsim_lib, case):
    dc.gradient_case(hostsim_lib, "cpu", *case)


def test_gradient_is_finite_on_the_denominator_clamp(hostsim_lib):
    dc.clamp_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("shape", dc.LOSS_SHAPES, ids=_ids)
def test_loss_pair_matches_the_ordered_float64_restatement(hostsim_lib, shape):
    dc.loss_case(hostsim_lib, "cpu", *shape)


def test_loss_without_a_valid_pixel_and_single_pixel(hostsim_lib):
    dc.loss_edge_cases(hostsim_lib, "cpu")


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    dc.refusal_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    dc.gradient_case(hostsim_lib, "cpu", *dc.GRAD_CASES[1])
    dc.loss_case(hostsim_lib, "cpu", *dc.LOSS_SHAPES[0])
    log = kc.launch_log(hostsim_lib)
    assert dc.KERNELS <= dc.launched_kernels(log), log
    assert "render_depth_fwd_kernel<3>" in log and "render_depth_bwd_kernel<3>" in log
