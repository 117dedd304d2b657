"""Measures how far hifihr_amd.lpips.LPIPS (HIP kernels) is from the float64 restatement of tests/lpips_ref.py, per input family of
tests/test_gpu_lpips.py and per conv_precision, next to r32 = the error of the same restatement run in float32 by torch on the CPU.
Writes profiles/lpips_precision.txt.  The test asserts HIP <= 64 x r32 on the direct kernels ("reference"); "fast" is recorded only.

usage: python tools/lpips_precision.py [--out profiles/lpips_precision.txt]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import torch
    import lpips_cases as lc
    from hifihr_amd.lpips import LPIPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_precision.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_precision needs a GPU: there is no fallback"
    lines = [f"LPIPS(net='alex', seed=0) on {torch.cuda.get_device_name(0)} against the float64 CPU restatement with the same weights (tools/lpips_precision.py).",
             "rel = largest relative error over the batch; r32 = the same for the restatement run in float32 by torch on the CPU; the test's bound is "
             f"rel <= {lc.E2E_FACTOR:.0f} x r32 on conv_precision='reference' (direct kernels); 'fast' (Winograd 3x3 layers) is recorded only.",
             "Parity with the `lpips` package and with the real weights is NOT measured here: neither is available.", "",
             f"{'family':12s} {'N x H x W':>14s} {'r32':>10s} | {'reference rel':>13s} {'ratio':>7s} | {'fast rel':>10s} {'ratio':>7s} | value[0] (float64)"]
    mods = {p: LPIPS(seed=0, conv_precision=p).cuda() for p in ("reference", "fast")}
    over = []
    for family, N, H, W in (("independent", 4, 224, 224), ("masked", 4, 224, 224), ("near", 4, 224, 224), ("independent", 3, 67, 95),
                            ("independent", 2, 31, 31), ("identical", 4, 224, 224)):
        in0, in1 = lc.e2e_inputs(family, N, H, W, seed=H if (H, W) != (31, 31) else 3)
        if family == "identical":
            zs = {p: float(m(in0.cuda(), in1.cuda()).abs().max()) for p, m in mods.items()}
            lines.append(f"{family:12s} {f'{N}x{H}x{W}':>14s} {'-':>10s} | max |value| reference {zs['reference']!r}, fast {zs['fast']!r} (the test requires exactly 0.0 on reference)")
            continue
        res = {p: lc.e2e_measure(m, in0, in1) for p, m in mods.items()}
        r32 = res["reference"][1]
        rr, rf = res["reference"][0], res["fast"][0]
        lines.append(f"{family:12s} {f'{N}x{H}x{W}':>14s} {r32:10.3e} | {rr:13.3e} {rr / r32:7.2f} | {rf:10.3e} {rf / r32:7.2f} | {float(res['reference'][3][0]):.6e}")
        if rr > lc.E2E_FACTOR * r32:
            over.append(f"FINDING: {family} {N}x{H}x{W} exceeds {lc.E2E_FACTOR:.0f} x r32 on the direct kernels (ratio {rr / r32:.1f})")
    lines += [""] + (over or [f"no family exceeds {lc.E2E_FACTOR:.0f} x r32 on the direct kernels"])
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
