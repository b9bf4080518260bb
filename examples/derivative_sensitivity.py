"""Screening by derivatives: the DGSM nu_i = E[(df/dz_i)^2] of V_cc, div_angle and T_c over the PEM-v0 priors from ONE pass of n
evaluations with the exact Jacobian, the bound it puts on the total Sobol' index beside the Saltelli estimate of that index (which
takes n (d + 2) evaluations), and the leading direction of each QoI's active subspace.

    python examples/derivative_sensitivity.py [n]

z_i is the coordinate the prior of input i is stated in (log10 x_i for the log-uniform inputs).  ST <= bound always holds; the bound
is tight (12 / pi^2 = 1.22 ST) where the QoI is linear in z_i and loose where it is strongly nonlinear.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402


def main(n: int = 1 << 16):
    res = drivers.derivative_sensitivity(n, seed=11, design='sobol')
    sob = drivers.sobol_indices(n, seed=11, design='sobol')
    names = res['inputs']
    assert names == list(sob['inputs'])
    print(f"{n} samples: {res['evaluations']} evaluations with the Jacobian (+ {res['pilot_evaluations']} for the centre) against "
          f"{n * (len(names) + 2)} of the Saltelli design; non-physical {res['non_physical']}, invalid {res['invalid']}, skipped {res['skipped']}")
    for q in ('V_cc', 'div_angle', 'T_c'):
        ST = torch.as_tensor(sob['ST'][q]).cpu()
        nu, se, bound, act = (res[k][q].cpu() for k in ('nu', 'nu_se', 'bound_ST', 'activity'))
        lam, W = res['eigenvalues'][q].cpu(), res['eigenvectors'][q].cpu()
        print(f"\n{q}: mean {res['mean'][q]:.6g}, variance {res['var'][q]:.6g}")
        print(f"{'input':>10s} {'nu':>12s} {'+-':>10s} {'ST bound':>10s} {'ST':>8s} {'activity':>10s}")
        for j in torch.argsort(bound, descending=True).tolist():
            print(f"{names[j]:>10s} {float(nu[j]):12.4e} {float(se[j]):10.2e} {float(bound[j]):10.4f} {float(ST[j]):8.4f} {float(act[j] / lam.sum()):10.4f}")
        share = float(lam[0] / lam.sum())
        w = W[:, 0] * torch.sign(W[torch.argmax(W[:, 0].abs()), 0])
        lead = ', '.join(f'{float(w[j]):+.2f} {names[j]}' for j in torch.argsort(w.abs(), descending=True).tolist()[:4])
        print(f"  leading active direction ({share:.1%} of the gradient's energy, standardised coordinates): {lead}")


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:2]))
