"""The backward kernels of the `lpips` loss term (csrc/lpips.hip) on the hostsim emulator through the C ABI: hifihr_lpips_tap_bwd
against float64 autograd of the restatement (tests/lpips_grad_ref.py), the tapless MaxPool2d(3, 2) pair against torch bit for bit,
the ScalingLayer repack's backward against its closed form -- and the backward-data product of the two AlexNet geometries that no other
test runs (11x11 stride 4 on the NHWC4 image, 5x5 pad 2)."""
import pytest

import kernel_cases as kc
import lpips_loss_cases as ll


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


# every (lanes per pixel, float4 per lane) instance, widths that leave lanes without channels (100, 260, 400), one and several pixels
@pytest.mark.parametrize("C", [8, 64, 100, 128, 192, 256, 260, 384, 400, 512])
@pytest.mark.parametrize("B,HW", [(1, 1), (3, 5), (1, 17)])
def test_lpips_tap_bwd(hostsim_lib, B, HW, C):
    ll.tap_bwd_case(hostsim_lib, "cpu", B, HW, C, seed=C + HW)


# more pixels than one pass of the capped grid covers, HW > 64 x (256 / G), for G = 16, 32, 64: several passes, a ragged last one
@pytest.mark.parametrize("B,HW,C", [(1, 1030, 64), (3, 520, 384), (1, 260, 256)])
def test_lpips_tap_bwd_many_pixel_blocks(hostsim_lib, B, HW, C):
    ll.tap_bwd_case(hostsim_lib, "cpu", B, HW, C, seed=C)


def test_lpips_tap_bwd_rejects(hostsim_lib):
    ll.tap_bwd_rejects_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("C", [4, 64, 192])
@pytest.mark.parametrize("H,W", [(3, 3), (7, 8), (15, 16)])
def test_lpips_maxpool(hostsim_lib, H, W, C):
    ll.pool_case(hostsim_lib, "cpu", 2, H, W, C, seed=H + C)


def test_lpips_maxpool_rejects(hostsim_lib):
    ll.pool_rejects_case(hostsim_lib, "cpu")


def test_image_scale_to_nhwc4_bwd(hostsim_lib):
    ll.scale_bwd_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("N,H,W,C,K,R,stride,pad", [(1, 31, 35, 4, 64, 11, 4, 2), (1, 7, 6, 64, 192, 5, 1, 2),
                                                    (2, 70, 77, 4, 64, 11, 4, 2)])      # the stem again: two samples, more than 64 pixels per phase
def test_alexnet_conv_backward_data(hostsim_lib, N, H, W, C, K, R, stride, pad):
    ll.conv_dgrad_case(hostsim_lib, "cpu", N, H, W, C, K, R, stride, pad, seed=R)
