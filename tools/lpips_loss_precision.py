"""Measures how far the backward of the `lpips` loss term (csrc/lpips.hip, hifihr_amd.lpips.LPIPS(differentiable=True)) is from float64
autograd of the restatement (tests/lpips_grad_ref.py): every kernel case and every end-to-end case of tests/test_gpu_lpips_loss.py, next
to r32 = the error of the same restatement run in float32 by torch on the CPU.  Writes profiles/lpips_loss_precision.txt.  The tests
assert HIP <= 64 x r32 (both as max |error| / max |float64 result|); a case beyond it is written down as a FINDING.

usage: python tools/lpips_loss_precision.py [--out profiles/lpips_loss_precision.txt]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import torch
    import lpips_loss_cases as ll
    from hifihr_amd._lib import get_lib
    from hifihr_amd.lpips import LPIPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_loss_precision.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_loss_precision needs a GPU: there is no fallback"
    lib, diff, metric = get_lib(), LPIPS(seed=0, differentiable=True).cuda(), LPIPS(seed=0).cuda()
    failed = []

    def run(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except AssertionError as e:
            failed.append(f"FINDING: {fn.__name__}{args[1:] if fn is not ll.e2e_grad_case else args[2:]}: {e}")

    for C in (8, 64, 100, 128, 192, 256, 260, 384, 400, 512):
        for B, HW in ((1, 1), (3, 5), (1, 17)):
            run(ll.tap_bwd_case, lib, "cuda", B, HW, C, seed=C + HW)
    for B, HW, C in ((1, 1030, 64), (3, 520, 384), (1, 260, 256), (32, 3025, 64), (32, 729, 192), (32, 169, 384), (32, 169, 256)):
        run(ll.tap_bwd_case, lib, "cuda", B, HW, C, seed=C)
    for H, W in ((3, 3), (7, 8), (15, 16)):
        for C in (4, 64, 192):
            run(ll.pool_case, lib, "cuda", 2, H, W, C, seed=H + C)
    run(ll.scale_bwd_case, lib, "cuda")
    for N, H, W in ((3, 35, 47), (2, 63, 67)):
        for family in ("independent", "near", "masked"):
            run(ll.e2e_grad_case, diff, metric, family, N, H, W, seed=H)
    lines = [f"backward of the `lpips` loss term on {torch.cuda.get_device_name(0)} against float64 autograd of the CPU restatement, seeded weights "
             "(tools/lpips_loss_precision.py).",
             "err = max |HIP - float64| / max |float64|; r32 = the same for the restatement run in float32 by torch on the CPU; the tests' bound is "
             f"err <= {ll.FACTOR:.0f} x r32.  The pool pair is compared bit for bit (0 / 0).", "",
             f"{'case':64s} {'err':>10s} {'r32':>10s} {'ratio':>8s}"]
    for what, e, r32 in ll.PRECISION:
        ratio = f"{e / r32:8.2f}" if r32 > 0 else ("    0.00" if e == 0 else "     inf")
        lines.append(f"{what:64s} {e:10.3e} {r32:10.3e} {ratio}")
    lines += [""] + (failed or [f"no case exceeds {ll.FACTOR:.0f} x r32; every exact comparison held"])
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
