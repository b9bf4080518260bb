"""Which pairs of inputs interact: second-order Sobol' indices of V_cc, div_angle and T_c at a fixed operating point
(P_b = 1e-5 Torr, V_a = 300 V, mdot_a = 5e-6 kg/s; the other 12 inputs over their priors), Saltelli design on the shifted Sobol'
sequence, one fused launch.

    python examples/second_order_indices.py [n_base] [n_pairs]

Prints, per QoI, the `n_pairs` pairs with the largest |S2| and the closure sum S1 + sum S2 (1 when nothing of third order is left).
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402
from hallthrusterpem_amd.batch import QOI_NAMES  # noqa: E402

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6}


def main(n_base: int = 1 << 20, n_pairs: int = 5):
    res = drivers.sobol_indices(n_base, seed=11, fixed=FIXED, design='sobol', second_order=True)
    names = res['inputs']
    print(f"{n_base} base samples, {len(names)} varied inputs, {res['evaluations']:.3g} evaluations; "
          f"non-physical {res['non_physical']}, invalid {res['invalid']}")
    for q in QOI_NAMES:
        S1, S2 = res['S1'][q], res['S2'][q]
        upper = S2.triu(1)
        sum_s1, sum_s2 = float(S1.sum()), float(upper.sum())
        print(f"\n{q}: centre {float(res['centre'][q]):.6g}, sum S1 = {sum_s1:.4f}, sum S2 = {sum_s2:.4f}, closure = {sum_s1 + sum_s2:.4f}")
        order = torch.argsort(upper.abs().flatten(), descending=True)[:n_pairs]
        for k in order.tolist():
            i, j = divmod(k, len(names))
            print(f'    {names[i]:>9s} x {names[j]:<9s} S2 = {float(S2[i, j]):+.4f}')


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:3]))
