"""Prints what RENDER_CONTRACT_C of tests/kernel_cases.py is made of: per kind, the worst err / ((sqrt(L) + K) max|ref|) of the renderer
contract's reference run in float32 against its float64 run over the emulator list, and four times that.  CPU only: python tools/render_contract_c.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import kernel_cases as kc  # noqa: E402
import test_hostsim_render_contract as rc  # noqa: E402

if __name__ == "__main__":
    worst = {}
    for case in rc.RENDER_CASES:
        for kind, v in kc.render_contract_measure([case]).items():
            if v > worst.get(kind, (0.0, None))[0]:
                worst[kind] = (v, case)
    for kind in kc.RENDER_CONTRACT_KINDS:
        v, case = worst.get(kind, (0.0, None))
        print(f"{kind:12s} {v:.2e} x 4 = {4 * v:.1e}   (in the table: {kc.LAYER_CONTRACT_C[kind][0]:.1e})   worst on {case}")
