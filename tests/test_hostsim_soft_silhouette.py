"""The soft silhouette and its losses (csrc/soft_sil.hip: hifihr_soft_sil_fwd / _bwd, hifihr_soft_sil_loss_fwd / _bwd) on the host
emulator, plus the host-only checks of the Python surface.  The cases are those of tests/test_gpu_soft_silhouette.py
(tests/soft_sil_cases.py); the reference is the float64 restatement of tests/soft_sil_ref.py."""
import pytest
import torch

import kernel_cases as kc
import soft_sil_cases as sc

_ids = lambda g: "-".join(str(v) for v in g)


@pytest.fixture(scope="module")
def hostsim_lib():
    return kc.build_hostsim()


def test_known_answers(hostsim_lib):
    sc.known_answers_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("case", sc.RANDOM_CASES, ids=_ids)
def test_random_meshes_match_the_restatement(hostsim_lib, case):
    sc.random_case(hostsim_lib, "cpu", *case)


def test_mano_topology_matches_the_restatement(hostsim_lib, synth_tables):
    sc.mano_case(hostsim_lib, "cpu", synth_tables, 64)


def test_outputs_are_fully_written_and_repeatable(hostsim_lib):
    sc.buffers_case(hostsim_lib, "cpu")


def test_refusals_leave_the_outputs_untouched(hostsim_lib):
    sc.refusal_case(hostsim_lib, "cpu")


@pytest.mark.parametrize("shape", sc.LOSS_SHAPES, ids=_ids)
def test_losses_match_the_float64_formulas(hostsim_lib, shape):
    sc.losses_case(hostsim_lib, "cpu", *shape)


def test_losses_take_a_float_mask(hostsim_lib):
    sc.losses_case(hostsim_lib, "cpu", 2, 17, mask_dtype=torch.float32)


def test_empty_image_gives_nan_like_iou(hostsim_lib):
    sc.losses_nan_case(hostsim_lib, "cpu")


def test_kernels_were_launched(hostsim_lib):
    kc.launch_log(hostsim_lib)
    sc.buffers_case(hostsim_lib, "cpu")
    sc.losses_case(hostsim_lib, "cpu", 1, 16)
    assert sc.KERNELS <= set(kc.launch_log(hostsim_lib))


# ---- Python surface, host only -------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from hifihr_amd import ops
    from hifihr_amd._lib import HifihrError
    with pytest.raises(HifihrError):
        ops.soft_silhouette(None, torch.zeros(1, 4, 3), torch.zeros(1, 4))
    with pytest.raises(HifihrError):
        ops.soft_sil_losses(torch.zeros(1, 1, 4, 4), torch.zeros(1, 4, 4), 1.0, 1.0)


def test_options_carry_the_defaults():
    import math
    import sys
    sys.path.insert(0, kc.REPO)
    import train_hrnet
    from hifihr_amd import ops, options
    a = options.make_args()
    assert (a.soft_silhouette, a.soft_sil_sigma, a.lambda_silhouette_soft, a.lambda_iou_soft) == (False, 1e-4, 0.005, 1e-3)
    assert (a.lambda_silhouette_soft, a.lambda_iou_soft) == (options._DEFAULTS["lambda_silhouette"], options._DEFAULTS["lambda_iou"])
    assert "sil_soft" not in a.losses and "iou_soft" not in a.losses
    assert ops.SOFT_SIL_SIGMA == 1e-4 and ops.soft_sil_default_blur(1e-4) == math.log(1.0 / 1e-4 - 1.0) * 1e-4
    # the front end builds the model with the option when asked, or when a term that reads re_sil_soft is requested
    assert train_hrnet.soft_silhouette_kwargs(a) == dict(soft_silhouette=False, soft_sil_sigma=1e-4)
    assert train_hrnet.soft_silhouette_kwargs(options.make_args(soft_silhouette=True, soft_sil_sigma=2e-4)) == dict(soft_silhouette=True, soft_sil_sigma=2e-4)
    for k in ("sil_soft", "iou_soft"):
        assert train_hrnet.soft_silhouette_kwargs(options.make_args(losses=a.losses + [k]))["soft_silhouette"] is True
    assert train_hrnet.build_args(train_hrnet.parse(["--soft_silhouette"])).soft_silhouette is True
    assert train_hrnet.build_args(train_hrnet.parse([])).soft_silhouette is False


def test_loss_function_needs_the_model_option():
    from hifihr_amd import options
    from hifihr_amd.losses import LossFunction
    args = options.make_args()
    for k in ("sil_soft", "iou_soft"):
        with pytest.raises(AssertionError, match="soft_silhouette"):
            LossFunction()({"segms_gt": torch.zeros(1, 4, 4, dtype=torch.int64)}, {}, [k], "FreiHand", args)
