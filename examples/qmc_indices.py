"""First-order and total Sobol' indices of V_cc, div_angle and T_c from a few thousand base samples: the Saltelli design on the
shifted Sobol' sequence (`design='sobol'`) beside the design of independent draws (`design='mc'`), both against a large run.

    python examples/qmc_indices.py [n_base] [n_shifts]

Prints, per QoI, the largest |S1 - reference| and |ST - reference| over the inputs and over `n_shifts` seeds for either design, and
the means' errors in units of one Monte-Carlo standard error sigma / sqrt(n_base).  The reference is a 2^20-point Sobol' run.
"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402
from hallthrusterpem_amd.batch import QOI_NAMES  # noqa: E402


def main(n_base: int = 4096, n_shifts: int = 4):
    ref = drivers.sobol_indices(1 << 20, seed=0, design='sobol', scramble=False)
    print(f"reference: {ref['evaluations']:.3g} evaluations of the unshifted sequence; inputs {ref['inputs']}")
    worst = {d: {k: {q: 0.0 for q in QOI_NAMES} for k in ('S1', 'ST', 'mean')} for d in ('mc', 'sobol')}
    for seed in range(1, n_shifts + 1):
        for design in ('mc', 'sobol'):
            res = drivers.sobol_indices(n_base, seed=seed, design=design)
            for q in QOI_NAMES:
                for k in ('S1', 'ST'):
                    worst[design][k][q] = max(worst[design][k][q], float((res[k][q] - ref[k][q]).abs().max()))
                se = float(torch.sqrt(ref['var'][q] / (2 * n_base)))          # the mean pools the A and B evaluations
                worst[design]['mean'][q] = max(worst[design]['mean'][q], abs(float(res['mean'][q] - ref['mean'][q])) / se)
    print(f'\nn_base = {n_base}, {n_shifts} seeds, {n_base * (len(ref["inputs"]) + 2)} evaluations per run; worst over inputs and seeds')
    print(f"{'':12s} {'|S1 - ref|':>23s} {'|ST - ref|':>23s} {'|mean - ref| / se':>23s}")
    print(f"{'':12s} " + ' '.join(f"{'mc':>11s} {'sobol':>11s}" for _ in range(3)))
    for q in QOI_NAMES:
        cells = ' '.join(f"{worst['mc'][k][q]:11.4f} {worst['sobol'][k][q]:11.4f}" for k in ('S1', 'ST', 'mean'))
        print(f'{q:12s} {cells}')


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:3]))
