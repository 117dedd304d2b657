"""Autograd-capable torch restatement of LPIPS(net="alex"), version 0.1, for the tests of the `lpips` loss term and of the backward
kernels of csrc/lpips.hip (runs on the CPU in float64 or float32).  tests/lpips_ref.py is the forward-only restatement (it detaches
its inputs); the constants come from there.

The one place where this is not plain autograd: the channel norm.  r = sqrt(sum_c f^2) has no derivative at an all-zero pixel (autograd
gives NaN); the kernels take the radial part of the gradient as 0 there (include/hifihr.h, hifihr_lpips_tap_bwd), and so does
`channel_norm`: torch.where on a clamped sum, so that the square root is never differentiated at 0.
"""
import torch
import torch.nn.functional as F

from lpips_ref import ALEX, SCALE, SHIFT

EPS = 1e-10


def channel_norm(f):
    """sqrt(sum_c f^2) over the last axis, keepdim, with a zero (not NaN) gradient at an all-zero pixel."""
    s = f.pow(2).sum(-1, keepdim=True)
    tiny = torch.finfo(f.dtype).tiny
    return torch.where(s > 0, s.clamp_min(tiny).sqrt(), torch.zeros_like(s))


def tap_grad_ref(f0, f1, w):
    """One tap on channels-last maps [B, HW, C] -> [B], differentiable with respect to f0 (f1 is detached: the target)."""
    n0 = f0 / (channel_norm(f0) + EPS)
    f1 = f1.detach()
    n1 = f1 / (channel_norm(f1) + EPS)
    return ((n0 - n1).pow(2) * w).sum(-1).mean(-1)


def tap_bwd_ref(f0, f1, w, gval, dtype):
    """-> gval[b] * d tap[b] / d f0, [B, HW, C] in `dtype`."""
    x = f0.to(dtype).clone().requires_grad_(True)
    tap_grad_ref(x, f1.to(dtype), w.to(dtype)).backward(gval.to(dtype))
    return x.grad


def lpips_alex_grad_ref(in0, in1, convs, lins, dtype=torch.float64, shift=SHIFT, scale=SCALE, record=None):
    """-> val [N] in `dtype`, differentiable with respect to in0 (a CPU tensor of `dtype`); in1 is the target.
    record: a dict that receives 'pre' (the five pre-activation maps of in0's half) and 'pool' (the two pool inputs of in0's half),
    detached unless record['graph'] is set."""
    keep = (lambda t: t) if (record is not None and record.get("graph")) else (lambda t: t.detach())
    sh = torch.tensor(shift, dtype=dtype).view(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=dtype).view(1, 3, 1, 1)
    N = in0.shape[0]
    x = torch.cat([(in0.to(dtype) - sh) / sc, (in1.detach().to(dtype) - sh) / sc])
    val = torch.zeros(N, dtype=dtype)
    for (w, b), lin, (_, _, _, stride, pad, pool) in zip(convs, lins, ALEX):
        if pool:
            if record is not None:
                record.setdefault("pool", []).append(keep(x[:N]))
            x = F.max_pool2d(x, 3, 2)
        z = F.conv2d(x, w.to(dtype), b.to(dtype), stride=stride, padding=pad)
        if record is not None:
            record.setdefault("pre", []).append(keep(z[:N]))
        x = F.relu(z)
        f = x.permute(0, 2, 3, 1).reshape(2 * N, -1, x.shape[1])
        val = val + tap_grad_ref(f[:N], f[N:], lin.to(dtype))
    return val


def lpips_value_and_grad(in0, in1, convs, lins, dtype, gval=None, shift=SHIFT, scale=SCALE, record=None):
    """-> (val [N], d sum_b gval[b] val[b] / d in0 [N,3,H,W]) in `dtype`; gval None: ones."""
    x = in0.detach().cpu().to(dtype).clone().requires_grad_(True)
    val = lpips_alex_grad_ref(x, in1.detach().cpu(), convs, lins, dtype, shift, scale, record)
    val.backward(torch.ones_like(val) if gval is None else gval.to(dtype))
    return val.detach(), x.grad
