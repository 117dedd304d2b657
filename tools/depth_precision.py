#!/usr/bin/env python3
"""Write profiles/depth_precision.txt: what the bounds of tests/depth_cases.py rest on.

  * forward: for every bit-equality case (tests/depth_cases.py KINDS at every size, the MANO topology at image_size 32) whether the kernel's
    depth has the bits of oracle/raster_oracle.c's zbuf (aa = 1) and of the float32 restatement (aa = 1, 2, 3), or else the count of
    differing elements and the largest distance in ulp;
  * gradient: per case of GRAD_CASES the kernel's error and the error of the same restatement evaluated in float32 on the CPU, both
    against float64 autograd as max-abs over max-abs-ref, and their ratio.  The test's bound is the float32 restatement's error times
    8 x the worst ratio found here (depth_cases.GRAD_WORST_RATIO).
Runs on the GPU when there is one, else on the host emulator (the file says which).

    python tools/depth_precision.py [--out profiles/depth_precision.txt]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_precision.txt"))
    cli = ap.parse_args()
    import depth_cases as dc
    import kernel_cases as kc
    from hifihr_amd.mano_tables import synthetic_mano_tables
    if torch.cuda.is_available():
        from hifihr_amd._lib import get_lib
        lib, device, where = get_lib(), "cuda", torch.cuda.get_device_name(0)
    else:
        lib, device, where = kc.build_hostsim(), "cpu", "host emulator (tests/hostsim)"
    lines = ["depth map: precision of csrc/depth.hip against the references of tests/depth_ref.py", f"kernels on: {where}", "",
             "forward, bit for bit against oracle/raster_oracle.c's zbuf (aa = 1) and the float32 restatement (aa = 1, 2, 3); hits exact",
             f"sizes: image_size x aa = {dc.SIZES}"]
    runs = [(kind, lambda k=kind: dc.bit_equality_case(lib, device, k)) for kind in dc.KINDS]
    runs.append(("mano, image_size 32, B = 2", lambda: dc.mano_bits_case(lib, device, synthetic_mano_tables(0))))
    for tag, fn in runs:
        try:
            fn()
            lines.append(f"  {tag:28s} 0 elements differ (0 ulp)")
        except AssertionError as e:                       # the assertion's text carries the count and the distance
            lines.append(f"  {tag:28s} DIFFERS: {str(e).splitlines()[0]}")
    lines += ["", "gradient: max|g - g64| / max|g64|, g64 = float64 autograd of the restatement with the kernel's face_id and hits as constants",
              f"{'H':>3s} {'aa':>3s} {'B':>2s} {'F':>3s} {'seed':>4s} {'coverage':>9s} {'kernel':>11s} {'float32':>11s} {'ratio':>7s}"]
    worst = 0.0
    for case in dc.GRAD_CASES:
        e = dc.grad_errors(lib, device, *case)
        worst = max(worst, e["ratio"])
        H, aa, B, F, seed = case
        lines.append(f"{H:3d} {aa:3d} {B:2d} {F:3d} {seed:4d} {e['coverage']:9.2f} {e['kernel']:11.3e} {e['f32']:11.3e} {e['ratio']:7.3f}")
    lines += [f"worst kernel / float32 ratio: {worst:.3f}",
              f"tests/depth_cases.py: GRAD_WORST_RATIO = {dc.GRAD_WORST_RATIO:g}, bound = {dc.GRAD_FACTOR:g} x the float32 restatement's error "
              "(8 x the worst ratio: the factor covers the summation-order freedom of the atomics, which one run does not sample)"]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(cli.out)), exist_ok=True)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
