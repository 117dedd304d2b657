"""Host side of the LPIPS feature, no GPU: the weight loader on both key layouts, the seeded initialisation, the refusals that need no
device, and the evaluation front-end's --lpips_weights flag (train_hrnet.make_evaluator) from weight files on disk."""
import os
import sys

import pytest
import torch

from test_gpu_lpips import _both_layouts, _seeded_tensors

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seeded_module_is_frozen_and_reproducible():
    from hifihr_amd.lpips import ALEX_LAYERS, LPIPS
    a, b, c = LPIPS(seed=0), LPIPS(seed=0), LPIPS(seed=1)
    assert not a.training and not a.train().training and not any(p.requires_grad for p in a.parameters())
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert not torch.equal(a.convs[0].weight, c.convs[0].weight)
    assert [tuple(m.weight.shape) for m in a.convs] == [(k, ci, r, r) for (_, _, ci, k, r, *_x) in ALEX_LAYERS]
    assert [p.numel() for p in a.lins] == [64, 192, 384, 256, 256] and all(float(p.min()) >= 0 for p in a.lins)
    # the stem filter the kernels read: the 3-channel parameter with a zero fourth plane
    assert torch.equal(a.stem_w4[:, :3], a.convs[0].weight) and float(a.stem_w4[:, 3].abs().max()) == 0.0
    assert "stem_w4" not in a.state_dict()
    with pytest.raises(NotImplementedError):
        LPIPS(net="vgg")
    with pytest.raises(ValueError):
        LPIPS(conv_precision="bf16")


def test_loader_on_both_key_layouts_and_missing_keys():
    from hifihr_amd.lpips import LPIPS, load_state_dict_lpips
    convs, lins = _seeded_tensors()
    two, one = _both_layouts(convs, lins)
    a = load_state_dict_lpips(LPIPS(seed=1), *two)
    b = load_state_dict_lpips(LPIPS(seed=2), *one)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters())) and torch.equal(a.stem_w4, b.stem_w4)
    for conv, (w, bias), p, lin in zip(a.convs, convs, a.lins, lins):
        assert torch.equal(conv.weight, w) and torch.equal(conv.bias, bias) and torch.equal(p, lin.reshape(-1))
    assert torch.equal(a.stem_w4[:, :3], convs[0][0]) and not any(p.requires_grad for p in a.parameters())
    c = LPIPS(seed=3)
    before = [p.clone() for p in c.parameters()]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        load_state_dict_lpips(c, {k: v for k, v in one[0].items() if k != "lin3.model.1.weight"})
    with pytest.raises(KeyError, match=r"features\.10\.weight"):
        load_state_dict_lpips(c, {k: v for k, v in two[0].items() if k != "features.10.weight"}, two[1])
    assert all(torch.equal(p, q) for p, q in zip(c.parameters(), before)), "a refused load changed the module"
    # scaling constants travel with the package's full state dict
    full = dict(one[0])
    full["scaling_layer.shift"] = torch.tensor([0.1, 0.2, 0.3]).view(1, 3, 1, 1)
    assert load_state_dict_lpips(LPIPS(), full).shift == pytest.approx((0.1, 0.2, 0.3))


def test_cpu_tensors_are_refused():
    from hifihr_amd._lib import HifihrError
    from hifihr_amd.lpips import LPIPS
    m, x = LPIPS(), torch.rand(1, 3, 64, 64)
    with pytest.raises(HifihrError):
        m(x, x.clone())


def test_front_end_flag_builds_the_evaluator_from_files(tmp_path):
    sys.path.insert(0, REPO)
    import train_hrnet
    from hifihr_amd import options
    convs, lins = _seeded_tensors()
    two, one = _both_layouts(convs, lins)
    torch.save(two[0], tmp_path / "alexnet.pth"); torch.save(two[1], tmp_path / "alex.pth"); torch.save(one[0], tmp_path / "lpips_full.pth")
    assert options.make_args().lpips_weights is None
    assert train_hrnet.build_args(train_hrnet.parse([])).lpips_weights is None
    assert train_hrnet.make_evaluator(train_hrnet.build_args(train_hrnet.parse([])), "cpu").lpips_fn is None          # nothing changes without the flag
    for paths in ([str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")], [str(tmp_path / "lpips_full.pth")]):
        args = train_hrnet.build_args(train_hrnet.parse(["--lpips_weights"] + paths))
        assert args.lpips_weights == paths
        ev = train_hrnet.make_evaluator(args, "cpu")
        fn = ev.lpips_fn
        assert fn is not None and fn is train_hrnet.make_evaluator(args, "cpu").lpips_fn                               # built once
        for conv, (w, bias), p, lin in zip(fn.convs, convs, fn.lins, lins):
            assert torch.equal(conv.weight, w) and torch.equal(conv.bias, bias) and torch.equal(p, lin.reshape(-1))
