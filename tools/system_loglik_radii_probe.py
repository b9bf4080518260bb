#!/usr/bin/env python3
"""Time the fused multi-QoI likelihood at several sweep radii (`pem_coupled_system_loglik_radii_f64_dev`: one model evaluation per
sample) against the composition it replaces -- one `pem_coupled_system_loglik_f64_dev` launch per radius, each with the
one-radius table of that radius, and the torch add of their results -- at n = 1.25e6, interleaved with device events.

    python tools/system_loglik_radii_probe.py [--n 1250000] [--reps 20] [--rounds 5] [--json OUT] [--txt OUT]

Tables (8 j_ion conditions x 40 angles x 3 radii, plus the 3 V_cc + 3 T + 2 u_ion x 7 conditions of the reference-shaped table of
tools/system_loglik_probe.py):
  radii        SystemLikelihood(sweep_radii=(0.55, 1.0, 1.37)): 120 j_ion records per condition, one launch
  composition  three SystemLikelihood(sweep_radius=r) with the 40 records of radius r; V_cc, T and u_ion ride in the first one
               only (their terms must be counted once), the other two hold the j_ion conditions at the same positions
  same size    one radius with three times the angles (120 records per condition at r = 1.0): what the one-radius launch takes
               on a table of the new launch's size -- the difference is the cost of the radius handling itself
The composition's sum and the new launch's result must agree (rtol 1e-10, equal NaN patterns: they differ by rounding only) before
anything is timed or written.  Two limits of the composition, neither met by the probe's prior draws: it decides `invalid` radius
by radius, and its zero weights (var_y = inf) turn a NaN or infinite model value of V_cc / T / u_ion into NaN instead of 0.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

RADII = (0.55, 1.0, 1.37)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_250_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--txt', default=None)
    a = ap.parse_args()
    import torch
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    from hallthrusterpem_amd.sampling import Design

    rng = np.random.default_rng(0)
    ne, na, R = 8, 40, len(RADII)
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    xj = op(ne)
    alpha = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, na))
    y, std = rng.lognormal(0, 1, (ne, R * na)), rng.uniform(0.3, 1.5, (ne, R * na))
    zq = np.array([0.0, 0.011, 0.02, 0.0399, 0.0401, 0.06, 0.08])
    others = {'V_cc': {'x': op(3), 'y': rng.uniform(15, 35, 3), 'var_y': np.ones(3)},
              'T': {'x': op(3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
              'uion': {'x': op(2), 'y': rng.uniform(1e3, 2e4, (2, 7)), 'var_y': np.full((2, 7), 1e6), 'loc': zq}}
    loc = np.stack([np.repeat(RADII, na), np.tile(alpha, R)], 1)
    jall = {'x': xj, 'y': y, 'var_y': std ** 2, 'loc': loc}
    s_radii = SystemLikelihood({**others, 'jion': jall}, sweep_radii=RADII)

    def at(r):
        cols = slice(r * na, (r + 1) * na)
        return {'x': xj, 'y': y[:, cols], 'var_y': std[:, cols] ** 2, 'loc': loc[cols]}
    # the composition: every table has the 16 conditions of the full one (sample i belongs to condition i mod 16 in all of them);
    # the V_cc / T / u_ion records are measured in the first table and given zero weight (1 / std = 0 adds -0.5 * 0 * 0) in the others
    silent = {q: dict(d, var_y=np.full_like(np.asarray(d['var_y'], dtype=np.float64), np.inf)) for q, d in others.items()}
    s_one = [SystemLikelihood({**(others if r == 0 else silent), 'jion': at(r)}, sweep_radius=RADII[r]) for r in range(R)]
    wide = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, R * na))
    s_same = SystemLikelihood({**others, 'jion': {'x': xj, 'y': y, 'var_y': std ** 2, 'loc': np.stack([np.ones(R * na), wide], 1)}},
                              sweep_radius=1.0)
    assert s_radii.n_cond == s_same.n_cond == 16 and all(s.n_cond == 16 for s in s_one) and s_radii.n_rec == s_same.n_rec

    dev = torch.device('cuda', torch.cuda.current_device())
    b = CoupledBatch(a.n, profile=False, thruster_qoi=False, sweep_radius=RADII[-1])
    Design(seed=2).fill(b.inputs)
    for j in range(3):                                              # the operating columns of sample i: those of condition i mod 16
        b.inputs[(0, 1, 6)[j]].copy_(torch.as_tensor(np.resize(s_radii.operating[:, j], a.n), device=dev))
    batches = [CoupledBatch(a.n, profile=False, thruster_qoi=False, sweep_radius=r) for r in RADII]
    for bb in batches:
        bb.inputs, bb.qoi, bb.invalid = b.inputs, b.qoi, b.invalid  # one set of inputs and outputs: only the radius differs
        bb._bind()
    out = {k: torch.empty(a.n, dtype=torch.float64, device=dev) for k in ('radii', 'r0', 'r1', 'r2', 'sum', 'same')}

    def composition():
        for r in range(R):
            batches[r].run_system_loglik(s_one[r], out=out[f'r{r}'])
        torch.add(out['r0'], out['r1'], out=out['sum'])
        out['sum'].add_(out['r2'])

    runs = {
        'pem_coupled_system_loglik_radii_f64_dev[3 radii x 40]': lambda: b.run_system_loglik(s_radii, out=out['radii']),
        '3 x pem_coupled_system_loglik_f64_dev[40] + add': composition,
        'pem_coupled_system_loglik_f64_dev[1 radius x 120]': lambda: batches[1].run_system_loglik(s_same, out=out['same']),
        'pem_coupled_system_loglik_f64_dev[1 radius x 40]': lambda: batches[0].run_system_loglik(s_one[0], out=out['r0']),
    }
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in runs.values():                                        # warm-up: code objects, LDS attribute, occupancy query
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got, want = out['radii'].cpu().numpy(), out['sum'].cpu().numpy()
    ok = np.isfinite(want)
    agree = np.isclose(got[ok], want[ok], rtol=1e-10, atol=1e-9)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and ok.any() and agree.all(), \
        f'the new launch differs from the composition in {int((~agree).sum())} of {int(ok.sum())} samples'
    times = {k: [] for k in runs}
    for _ in range(a.rounds):                                       # interleaved: each round times every entry once
        for k, fn in runs.items():
            ev0.record()
            for _ in range(a.reps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) * 1e3 / a.reps)
    res = {'n': a.n, 'reps': a.reps, 'rounds': a.rounds, 'radii': RADII,
           'table': {'n_cond': s_radii.n_cond, 'n_rec': s_radii.n_rec, 'n_rec_one_radius': s_one[0].n_rec},
           'agreement_with_composition': {'finite': int(ok.sum()), 'within_rtol_1e-10': int(agree.sum()),
                                          'nan_pattern_equal': bool(np.array_equal(np.isnan(got), np.isnan(want)))},
           'us_per_launch': {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()}}
    keys = list(runs)
    med = lambda k: res['us_per_launch'][k]['median']                                                    # noqa: E731
    res['new_over_composition'] = med(keys[0]) / med(keys[1])
    res['new_over_same_size_one_radius'] = med(keys[0]) / med(keys[2])
    print(json.dumps(res, indent=1))
    for path in (a.json, a.txt):
        if path:
            Path(path).parent.mkdir(parents=True, exist_ok=True)
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1) + '\n')
    if a.txt:
        lines = [f'system_loglik_radii_probe: n = {a.n}, {a.rounds} interleaved rounds x {a.reps} launches, radii {RADII}',
                 f'table: {s_radii.n_cond} conditions, {s_radii.n_rec} records ({s_one[0].n_rec} in a one-radius table)', '',
                 f'{"entry":<58} {"median us":>10} {"min":>8} {"max":>8}   per round']
        for k in keys:
            v = res['us_per_launch'][k]
            lines.append(f'{k:<58} {v["median"]:>10.1f} {v["min"]:>8.1f} {v["max"]:>8.1f}   ' + ' '.join(f'{t:.1f}' for t in times[k]))
        lines += ['', f'new launch / composition                = {res["new_over_composition"]:.3f}',
                  f'new launch / one radius, same-size table = {res["new_over_same_size_one_radius"]:.3f}',
                  f'agreement with the composition: {res["agreement_with_composition"]}']
        Path(a.txt).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
