"""Sobol' indices of V_cc, thrust, ion velocity at the channel exit and ion current density on axis over a background-pressure
sweep: the study of scripts/pem_v0/sobol.py (compute_indices) and the table its spt100_sobol plots, as text.

    python examples/sobol_sweep.py [n_base]
    python examples/sobol_sweep.py --surrogate [n_base]

--surrogate trains a small component chain on the thruster test double and runs the study of V_cc, T and uion twice on the same
design rows: around the model, and around the chain as the reference's model() does (sobol.py:70-98).  It prints both sets of
indices side by side with their standard errors, and per QoI the largest |S1 difference| and |ST difference| in units of the model
run's standard error: how far the fit, not the estimator, moves the indices.
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from hallthrusterpem_amd import drivers  # noqa: E402

Z = 1.96                                   # 95 % bars, st.norm.ppf(0.975) as sobol.py:129
SURROGATE_VARIED = ('P_b', 'T_e', 'V_vac', 'Pstar', 'P_T', 'mdot_a', 'a_1')
SURROGATE_QOIS = ('V_cc', 'T', 'uion')


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


def train_chain(n_refine: int = 48):
    """a chain over the seven inputs the two groups vary; V_a and the plume's inputs sit at their nominal values"""
    from hallthrusterpem_amd import sobol as study
    from hallthrusterpem_amd.chain import ChainedSurrogate
    fixed = {k: v for k, v in study.PEM_V0_NOMINAL.items() if k not in SURROGATE_VARIED}
    chain = ChainedSurrogate(SURROGATE_VARIED, fixed, max_level=3, u_ion=True, field=False)
    for it in range(n_refine):
        chain.refine_step(num_refine=500, seed=it)
    return chain


def in_standard_errors(diff, se):
    """(largest |diff| / se over the indices with se > 0, largest |diff| over the others): an index the model gives exactly (the
    test double's T does not depend on a_1, its u_ion on neither mdot_a nor a_1) has no standard error to measure in"""
    diff, se = np.abs(np.asarray(diff)), np.asarray(se)
    on = se > 0
    return (float(np.max(diff[on] / se[on])) if on.any() else 0.0), (float(np.max(diff[~on])) if (~on).any() else 0.0)


def surrogate_main(n_base: int = 100_000, n_refine: int = 48):
    chain = train_chain(n_refine)
    print(f'chain trained with {n_refine} refinements: model evaluations per component {chain.model_evals}')
    model = drivers.sobol_sweep(n_base, qois=SURROGATE_QOIS, seed=0)
    surr = drivers.sobol_sweep(n_base, qois=SURROGATE_QOIS, seed=0, surrogate=chain)
    print(f"{surr['evaluations']:.3g} surrogate evaluations, {surr['extrapolated']} with the V_cc coordinate outside the thruster table's "
          f"domain, {surr['non_physical']} non-physical")
    for q in SURROGATE_QOIS:
        m, s = model[q], surr[q]
        print(f'\n{q}: model | surrogate, S1 +- se / ST +- se')
        print(f"{'P_b [Torr]':>11s} " + ' '.join(f'{k:>54s}' for k in m['inputs']))
        for p, pb in enumerate(model['P_b']):
            cells = []
            for i in range(len(m['inputs'])):
                one = lambda r: (f"{float(r['S1'][p, i]):+.3f}+-{float(r['S1_se'][p, i]):.3f}/"                    # noqa: E731
                                 f"{float(r['ST'][p, i]):.3f}+-{float(r['ST_se'][p, i]):.3f}")
                cells.append(f'{one(m)} | {one(s)}')
            print(f'{pb:11.3e} ' + ' '.join(f'{c:>54s}' for c in cells))
        d1, e1 = in_standard_errors((s['S1'] - m['S1']).cpu().numpy(), m['S1_se'].cpu().numpy())
        dt, et = in_standard_errors((s['ST'] - m['ST']).cpu().numpy(), m['ST_se'].cpu().numpy())
        print(f'{q}: largest |S1 difference| {d1:.2f} se, largest |ST difference| {dt:.2f} se (the model run\'s standard errors); '
              f"largest absolute differences {float((s['S1'] - m['S1']).abs().max()):.2e} / {float((s['ST'] - m['ST']).abs().max()):.2e}; "
              f'where the model run has no standard error (an index it gives exactly): {e1:.2e} / {et:.2e}')


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--surrogate']
    n = int(args[0]) if args else 100_000
    if '--surrogate' in sys.argv[1:]:
        surrogate_main(n)
    else:
        main(n)
