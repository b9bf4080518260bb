"""Which input drives which part of the plume: first-order and total Sobol' indices of log10 j_ion at each of the 91 angles of the
sweep, at a fixed operating point (P_b = 1e-5 Torr, V_a = 300 V, mdot_a = 5e-6 kg/s; the other 12 inputs over their priors), Saltelli
design on the shifted Sobol' sequence, one fused launch.

    python examples/sobol_profile.py [n_base]

Prints, per input, the variance-weighted aggregates GS1 / GST over the profile and the angle ranges (degrees) where the input has the
largest total index of all.
"""
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}


def ranges(mask, degrees):
    """'0-12, 40-41': the runs of consecutive angles where `mask` holds"""
    out, start = [], None
    for k, m in enumerate(list(mask) + [False]):
        if m and start is None:
            start = k
        elif not m and start is not None:
            out.append(f'{degrees[start]:.0f}' if k - 1 == start else f'{degrees[start]:.0f}-{degrees[k - 1]:.0f}')
            start = None
    return ', '.join(out) or '-'


def main(n_base: int = 1 << 18):
    res = drivers.sobol_profile(n_base, seed=11, fixed=FIXED, design='sobol')
    names, ST = res['inputs'], res['ST']
    degrees = (res['angles'] * (180.0 / math.pi)).tolist()
    print(f"{n_base} base samples, {len(names)} varied inputs, {res['evaluations']:.3g} evaluations of the profile "
          f"(+ {res['pilot_evaluations']} for the centre); non-physical {res['non_physical']}, invalid {res['invalid']}")
    print(f"largest standard error of an S1: {float(res['S1_se'].max()):.4f}, of an ST: {float(res['ST_se'].max()):.4f}; "
          f"sum GS1 = {float(res['GS1'].sum()):.4f}")
    leader = torch.argmax(ST, dim=1).tolist()
    print(f"\n{'input':>10s} {'GS1':>8s} {'GST':>8s}   leads (largest ST) at angles [deg]")
    for j in torch.argsort(res['GST'], descending=True).tolist():
        print(f"{names[j]:>10s} {float(res['GS1'][j]):8.4f} {float(res['GST'][j]):8.4f}   {ranges([lead == j for lead in leader], degrees)}")


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:2]))
