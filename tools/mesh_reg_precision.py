#!/usr/bin/env python3
"""Write profiles/mesh_reg_precision.txt: for every case of tests/mesh_reg_cases.py that is compared with the float64 restatement, the
error of the same restatement in float32 (torch, on the CPU) and the error of the kernels, both as a fraction of the largest reference
magnitude.  Runs on the GPU when there is one, else on the host emulator.

    python tools/mesh_reg_precision.py [--out profiles/mesh_reg_precision.txt]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_reg_precision.txt"))
    cli = ap.parse_args()
    import kernel_cases as kc
    import mesh_reg_cases as mc
    from hifihr_amd.mano_tables import synthetic_mano_tables
    if torch.cuda.is_available():
        from hifihr_amd._lib import get_lib
        lib, device, where = get_lib(), "cuda", torch.cuda.get_device_name(0)
    else:
        lib, device, where = kc.build_hostsim(), "cpu", "host emulator (tests/hostsim)"
    for case in mc.RANDOM_CASES:
        mc.random_case(lib, device, *case)
    mc.mano_case(lib, device, synthetic_mano_tables(0))
    mc.fan_case(lib, device)
    mc.isolated_vertex_case(lib, device)
    lines = ["mesh regularisers: error against the float64 restatement (tests/mesh_reg_ref.py), as a fraction of the largest reference magnitude",
             f"kernels on: {where}; float32 = the same restatement run by torch in float32 on the CPU",
             f"bound of the tests: kernel <= max({mc.KERNEL_OVER_F32:g} x float32, {mc.FLOOR:g})", "",
             f"{'case':28s} {'out float32':>12s} {'out kernel':>12s} {'grad float32':>13s} {'grad kernel':>12s}"]
    for tag, _, o32, ok, g32, gk in mc.PRECISION:
        lines.append(f"{tag:28s} {o32:12.2e} {ok:12.2e} {g32:13.2e} {gk:12.2e}")
    text = "\n".join(lines)
    print(text)
    with open(cli.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
