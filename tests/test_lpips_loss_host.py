"""Host side of the `lpips` loss term, no GPU: the name and its weight, the module's keyword and the refusals that need no device."""
import inspect

import pytest
import torch


def test_term_and_option_exist():
    from hifihr_amd import losses, options
    assert "lpips" in losses.TERMS
    assert options._DEFAULTS["lambda_lpips"] == 0.01 and options.make_args().lambda_lpips == 0.01
    assert options.make_args(lambda_lpips=0.5).lambda_lpips == 0.5
    assert "lpips" not in options.make_args().losses and "lpips" not in options.baseline_config2_args().losses       # opt-in by name
    sig = inspect.signature(losses.LossFunction.__init__)
    assert list(sig.parameters)[-1] == "lpips" and sig.parameters["lpips"].default is None
    assert losses.LossFunction().lpips_loss is None                                                                 # built on first use


def test_module_keyword_and_refusals():
    from hifihr_amd._lib import HifihrError
    from hifihr_amd.lpips import LPIPS
    plain, diff = LPIPS(), LPIPS(differentiable=True)
    assert plain.differentiable is False and diff.differentiable is True
    assert all(torch.equal(p, q) for p, q in zip(plain.parameters(), diff.parameters()))                           # the same seeded weights
    assert not diff.training and not diff.train().training and not any(p.requires_grad for p in diff.parameters())
    x = torch.rand(1, 3, 64, 64)
    g = x.clone().requires_grad_(True)
    for m in (plain, diff):
        with pytest.raises(HifihrError):
            m(x, x.clone())                                  # CPU tensors
    with pytest.raises(HifihrError):
        plain(g, x)                                          # the default module: nothing to differentiate on the host either
    with pytest.raises(NotImplementedError):
        diff(x, g)                                           # the target is a constant
    with torch.no_grad(), pytest.raises(HifihrError):
        diff(x, g)                                           # ... no gradient is recorded: only the device is missing


def test_bindings_exist():
    from hifihr_amd._lib import HifihrLib
    for name in ("lpips_tap_bwd", "lpips_maxpool_fwd", "lpips_maxpool_bwd", "image_scale_to_nhwc4_bwd"):
        assert callable(getattr(HifihrLib, name))
    from hifihr_amd import ops
    assert callable(ops.lpips_alex) and callable(ops.lpips_tap_bwd) and callable(ops.lpips_maxpool_bwd)
