#!/usr/bin/env python3
"""The yardstick of the open2d_terms bounds (tests/open2d_cases.py): the error the float32 evaluation of the restatement
(tests/open2d_ref.py) makes against its float64 evaluation, over the test's own case list, on the CPU.  No kernel runs here.

    python tools/open2d_precision.py [--out profiles/open2d_precision.txt]

Prints one line per case and the worst figure per output and for the gradient: F32_WORST_OUT / F32_WORST_GRAD of tests/open2d_cases.py."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import open2d_cases as oc
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "open2d_precision.txt"))
    cli = ap.parse_args()
    lines = ["float32 restatement against float64 restatement (tests/open2d_ref.py), relative errors, CPU",
             "outputs: |x32 - x64| / |x64|; gradient: max |g32 - g64| / max |g64| of the case; 0 where both are exactly 0",
             f"{'case':34s} {'open_2dj':>11s} {'open_bone_direc':>16s} {'open_2dj_de':>12s} {'gradient':>11s}"]
    worst, worst_g = [0.0, 0.0, 0.0], 0.0
    for case in oc.TERM_CASES:
        outs, g = oc.f32_errors(*case)
        lines.append(f"{str(case):34s} {outs[0]:11.3e} {outs[1]:16.3e} {outs[2]:12.3e} {g:11.3e}")
        worst = [max(a, b) for a, b in zip(worst, outs)]
        worst_g = max(worst_g, g)
    lines.append(f"{'worst':34s} {worst[0]:11.3e} {worst[1]:16.3e} {worst[2]:12.3e} {worst_g:11.3e}")
    lines.append(f"F32_WORST_OUT = ({worst[0]:.3e}, {worst[1]:.3e}, {worst[2]:.3e})   F32_WORST_GRAD = {worst_g:.3e}   "
                 f"(the tests allow {oc.FACTOR:g} x these)")
    text = "\n".join(lines)
    print(text)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
