#!/usr/bin/env python3
"""Record the precision of the one-launch keypoint fit (csrc/mano_fit.hip) on every kernel case of tests/mano_fit_cases.py: per compared
quantity the kernel's error against the float64 restatement (tests/mano_fit_ref.py), the float32 restatement's error on the same case, the
bound the tests hold (8 x the latter, with a floor of 8 float32 roundings of the quantity's scale) and the ratio kernel / restatement.

    python tools/mano_fit_precision.py [--device cuda | cpu] [--out profiles/mano_fit_precision.txt]

--device cuda runs the product library on the MI355X (with the 151-iteration cases); --device cpu runs the emulator build of the same
sources with the iteration counts of tests/test_hostsim_mano_fit.py."""
import argparse
import contextlib
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mano_fit_precision.txt"))
    cli = ap.parse_args()
    import dataclasses
    import numpy as np
    import kernel_cases as kc
    import mano_fit_cases as fc
    from hifihr_amd.mano_tables import synthetic_mano_tables
    synth = synthetic_mano_tables(0)
    g = dict(np.load(os.path.join(REPO, "tests", "golden", "mano_dense.npz")))
    dense = dataclasses.replace(synth, weights=g["weights"], hands_components=g["hands_components"], hands_mean=g["hands_mean"])
    tables = {"synth": synth, "dense": dense}
    if cli.device == "cuda":
        from hifihr_amd._lib import get_lib
        lib, counts = get_lib(), (1, 5, 151)
    else:
        lib, counts = kc.build_hostsim(), (1, 5)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        for case in fc.EVAL_CASES:
            fc.eval_case(lib, cli.device, tables[case[6]], *case[:6])
        for with3d in (False, True):
            for iters in counts:
                out, r64, c = fc.trajectory_case(lib, cli.device, synth, iters, with3d=with3d)
                if iters == 151:
                    fc.recovery_check(out, r64, c)
    rows = buf.getvalue().splitlines()
    ratios = [float(r.rsplit(" ", 1)[1]) for r in rows if "ratio to the restatement" in r and not r.endswith(("inf", "nan"))]
    head = [f"keypoint fit: error against the float64 restatement per compared quantity ({cli.device}; every line passed its bound)",
            f"command: python tools/mano_fit_precision.py --device {cli.device}",
            f"{len(ratios)} quantities; ratio kernel error / float32-restatement error: median {sorted(ratios)[len(ratios) // 2]:.2f}, "
            f"largest {max(ratios):.2f} (the tests allow {fc.FACTOR:.0f}, or the floor of {fc.FLOOR_ROUNDINGS} float32 roundings of the quantity's scale where that is larger)", ""]
    with open(cli.out, "w") as fh:
        fh.write("\n".join(head + rows) + "\n")
    print("\n".join(head))
    print("wrote", cli.out)


if __name__ == "__main__":
    main()
