"""LPIPS kernel SOURCES (csrc/lpips.hip) on the hostsim emulator through the C ABI: the tap kernel against a float64 restatement
(tests/lpips_ref.py), the tapless MaxPool2d(3, 2) against torch bit for bit, the ScalingLayer repack to 1 ulp -- and the two
convolution geometries of the AlexNet trunk that no other test exercises (11x11 stride 4 on the NHWC4 image, 5x5 pad 2)."""
import pytest

import kernel_cases as kc
import lpips_cases as lc


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


# (B, HW, C, identical sample): B > 1 -> the last sample has f1 == f0; the one-sample shapes run with and without
@pytest.mark.parametrize("B,HW,C,same", [(2, 15 * 15, 64, 1), (3, 7 * 7, 192, 2), (1, 3 * 3, 384, None), (1, 3 * 3, 384, 0),
                                         (2, 5 * 3, 256, 1), (1, 1, 4, None), (1, 1, 4, 0)])
def test_lpips_tap(hostsim_lib, B, HW, C, same):
    lc.tap_case(hostsim_lib, "cpu", B, HW, C, seed=C + HW, identical_sample=same)


def test_lpips_tap_other_widths(hostsim_lib):
    """every (lanes per pixel, float4 per lane) instance of the kernel, at widths that leave some lanes without channels"""
    for C in (8, 100, 128, 176, 260, 320, 448):
        lc.tap_case(hostsim_lib, "cpu", 2, 5, C, seed=C, identical_sample=1)


def test_lpips_tap_many_pixel_blocks(hostsim_lib):
    """more pixels than one pass of the largest grid covers (64 workgroups x 4 pixels at C = 256): several passes, a ragged last one"""
    lc.tap_case(hostsim_lib, "cpu", 1, 64 * 4 * 2 + 3, 256, seed=3)


def test_lpips_tap_rejects(hostsim_lib):
    lc.tap_rejects_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("N,H,W,C", [(2, 15, 15, 64), (1, 7, 9, 8), (1, 3, 3, 4)])
def test_maxpool_notap(hostsim_lib, N, H, W, C):
    lc.pool_notap_case(hostsim_lib, "cpu", N, H, W, C, seed=H + C)


def test_maxpool_notap_rejects(hostsim_lib):
    lc.pool_rejects_case(hostsim_lib, "cpu")


def test_image_scale_to_nhwc4(hostsim_lib):
    lc.scale_repack_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", [(1, 31, 35, 4, 64, 11, 4, 2), (1, 7, 6, 64, 192, 5, 1, 2)])
def test_alexnet_conv_geometries(hostsim_lib, N, H, W, C, K, R, stride, pad):
    lc.conv_bias_relu_contract_case(hostsim_lib, "cpu", N, H, W, C, K, R, stride, pad, seed=R)
