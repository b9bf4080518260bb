"""Sobol' indices of V_cc, thrust, ion velocity at the channel exit and ion current density on axis over a background-pressure
sweep: the study of scripts/pem_v0/sobol.py (compute_indices) and the table its spt100_sobol plots, as text.

    python examples/sobol_sweep.py [n_base]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402

Z = 1.96                                   # 95 % bars, st.norm.ppf(0.975) as sobol.py:129


def main(n_base: int = 100_000):
    res = drivers.sobol_sweep(n_base, seed=0)
    print(f"{res['evaluations']:.3g} model evaluations; rejected plume draws per pressure {res['jion']['rejected'].tolist()}")
    for q in ('V_cc', 'T', 'uion', 'jion'):
        r = res[q]
        print(f'\n{q}: S1 / ST +- {Z} se')
        print(f"{'P_b [Torr]':>11s} " + ' '.join(f'{k:>25s}' for k in r['inputs']))
        for p, pb in enumerate(res['P_b']):
            cells = [f"{float(r['S1'][p, i]):+.3f}+-{Z * float(r['S1_se'][p, i]):.3f} / {float(r['ST'][p, i]):.3f}+-{Z * float(r['ST_se'][p, i]):.3f}"
                     for i in range(len(r['inputs']))]
            print(f'{pb:11.3e} ' + ' '.join(f'{c:>25s}' for c in cells))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100_000)
