"""The HO-3D device-path extras on the host emulator: hifihr_ho3d_keypoints, hifihr_ho3d_depth_crop (csrc/augment.hip) and
hifihr_depth_points (csrc/depth_points.hip).  The cases are those of tests/test_gpu_ho3d_extras.py (tests/ho3d_extras_cases.py)."""
import pytest

import ho3d_extras_cases as hc
import kernel_cases as kc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


@pytest.mark.parametrize("case", hc.DET_CASES, ids=_ids)
def test_detections_go_through_the_crop_window(hostsim_lib, case):
    hc.detections_case(hostsim_lib, "cpu", *case)


def test_keypoint_refusals_and_indices_outside_the_cache(hostsim_lib):
    hc.keypoints_refusal_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("S", hc.DEPTH_SIZES)
@pytest.mark.parametrize("frame", hc.DEPTH_FRAMES, ids=_ids)
def test_depth_crop_is_pillows_nearest_resize(hostsim_lib, frame, S):
    hc.depth_crop_case(hostsim_lib, "cpu", *frame, S)


def test_depth_crop_refusals(hostsim_lib):
    hc.depth_crop_refusal_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("P", hc.SELECT_P)
@pytest.mark.parametrize("shape", hc.SELECT_SHAPES, ids=_ids)
def test_point_selection_matches_the_restatement(hostsim_lib, shape, P):
    hc.selection_case(hostsim_lib, "cpu", *shape, P)


@pytest.mark.parametrize("with_origin", [False, True])
@pytest.mark.parametrize("kind", hc.K_KINDS)
def test_back_projection_matches_float64(hostsim_lib, kind, with_origin):
    hc.backprojection_case(hostsim_lib, "cpu", kind, with_origin)


def test_depth_points_refusals(hostsim_lib):
    hc.depth_points_refusal_case(hostsim_lib, "cpu")


def test_closed_loop_points_lie_on_the_rendered_mesh(hostsim_lib):
    hc.closed_loop_case(hostsim_lib, "cpu", hc.lib_surface_d2(hostsim_lib, "cpu"))


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    hc.detections_case(hostsim_lib, "cpu", 1, False)
    hc.depth_crop_refusal_case(hostsim_lib, "cpu")
    hc.depth_points_refusal_case(hostsim_lib, "cpu")
    log = set(kc.launch_log(hostsim_lib))
    assert hc.KERNELS <= log, log
