#!/usr/bin/env python3
"""Time the fused multi-QoI likelihood launch (`pem_coupled_system_loglik_f64_dev`) next to the j_ion-only fused launch
(`pem_coupled_loglik_f64_dev`) at n = 1.25e6, interleaved A/B with device events.

    python tools/system_loglik_probe.py [--n 1250000] [--reps 20] [--rounds 5] [--json OUT]

Tables (8 j_ion conditions x 40 angles in every one):
  jion      the 8 x 40 j_ion records alone, run by both launches (the system launch's answer is bit-identical: checked)
  system    SystemLikelihood with those 8 j_ion conditions + 3 V_cc + 3 T + 2 u_ion conditions x 7 positions (16 conditions;
            each sample sees its own condition's records, as in the reference's `System` calibration)
  stress    a hand-made table in which each of the 8 conditions holds its 40 j_ion records AND 1 V_cc, 1 T and 7 u_ion records:
            every sample pays the whole epilogue
  ablation  the same at the LDS footprint of the 8 x 40 j_ion table (8 x (32 j_ion + 9 others) records, the 41-record stride of
            pem_coupled_loglik_f64_dev's table), next to pem_coupled_loglik_f64_dev on the 8 x 32 j_ion records alone: the
            epilogue's own cost at equal occupancy
Resident workgroups per CU follow from LDS: 160 KiB over (69 696 B of profile tiles and tables + the measurement table).
"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1_250_000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd.batch import CoupledBatch
    from hallthrusterpem_amd.likelihood import JionLikelihood, SystemLikelihood
    from hallthrusterpem_amd.sampling import Design

    rng = np.random.default_rng(0)
    ne, na = 8, 40
    x = np.stack([10.0 ** rng.uniform(-6, -4.5, ne), rng.uniform(250, 350, ne), rng.uniform(4e-6, 6e-6, ne)], 1)
    alpha = np.sort(rng.uniform(-np.pi / 2, np.pi / 2, na))
    y, std = rng.lognormal(0, 1, (ne, na)), rng.uniform(0.3, 1.5, (ne, na))
    jdata = {'x': x, 'y': y, 'var_y': std ** 2, 'loc': np.stack([np.ones(na), alpha], 1)}
    jl = JionLikelihood(np.broadcast_to(alpha, (ne, na)), y, std)
    s_j = SystemLikelihood({'jion': jdata})
    zq = np.array([0.0, 0.011, 0.02, 0.0399, 0.0401, 0.06, 0.08])
    op = lambda k: np.stack([10.0 ** rng.uniform(-6, -4.5, k), rng.uniform(250, 350, k), rng.uniform(4e-6, 6e-6, k)], 1)  # noqa: E731
    s_sys = SystemLikelihood({
        'V_cc': {'x': op(3), 'y': rng.uniform(15, 35, 3), 'var_y': np.ones(3)},
        'T': {'x': op(3), 'y': rng.uniform(0.05, 0.1, 3), 'var_y': np.full(3, 1e-4)},
        'uion': {'x': op(2), 'y': rng.uniform(1e3, 2e4, (2, 7)), 'var_y': np.full((2, 7), 1e6), 'loc': zq},
        'jion': jdata})
    dev = torch.device('cuda', torch.cuda.current_device())
    u_rec = s_sys.rec.cpu().numpy()[s_sys.span.cpu().numpy()[s_sys.conditions['uion'].start, _lib.SYS_UION, 0]:][:7]

    def every_kind(jlik):
        """each condition of a j_ion-only SystemLikelihood given 1 V_cc, 1 T and the 7 u_ion records as well"""
        rec_j, span_j = jlik.rec.cpu().numpy(), jlik.span.cpu().numpy()
        blocks, span = [], np.zeros((ne, 4, 2), dtype=np.int32)
        first = 0
        for c in range(ne):
            f0, cnt = span_j[c, _lib.SYS_JION]
            parts = [(_lib.SYS_JION, rec_j[f0:f0 + cnt]), (_lib.SYS_VCC, np.array([[0.0, 25.0, 1.0, 0.0]])),
                     (_lib.SYS_T, np.array([[0.0, 0.08, 100.0, 0.0]])), (_lib.SYS_UION, u_rec)]
            for kind, r in parts:
                span[c, kind] = (first, r.shape[0])
                blocks.append(r)
                first += r.shape[0]
            if first % 2 == 0:
                blocks.append(np.zeros((1, 4)))
                first += 1
        return SimpleNamespace(sweep_radius=1.0, uion_grid=s_sys.uion_grid, n_cond=ne, n_rec=first,
                               rec=torch.as_tensor(np.concatenate(blocks), device=dev), span=torch.as_tensor(span, device=dev),
                               n_node=s_sys.n_node, node=s_sys.node)

    s_stress = every_kind(s_j)
    na_small = 32
    jd32 = dict(jdata, y=y[:, :na_small], var_y=std[:, :na_small] ** 2, loc=jdata['loc'][:na_small])
    jl32 = JionLikelihood(np.broadcast_to(alpha[:na_small], (ne, na_small)), y[:, :na_small], std[:, :na_small])
    s_abl = every_kind(SystemLikelihood({'jion': jd32}))
    base_lds = 69696
    lds = {'jion 8x40': base_lds + ne * (na | 1) * 32, 'jion 8x32': base_lds + ne * (na_small | 1) * 32}
    for key, t in (('system', s_sys), ('stress', s_stress), ('ablation', s_abl)):
        lds[key] = base_lds + t.n_rec * 32 + t.n_cond * 32 + max(t.n_node, 2) * 8

    b = CoupledBatch(a.n, profile=False, thruster_qoi=False)
    Design(seed=2).fill(b.inputs)
    out = {k: torch.empty(a.n, dtype=torch.float64, device=dev) for k in ('loglik', 'sys_j', 'sys', 'stress', 'l32', 'abl')}
    runs = {
        'pem_coupled_loglik_f64_dev[jion 8x40]': lambda: b.run_loglik(jl, out=out['loglik']),
        'pem_coupled_system_loglik_f64_dev[jion 8x40]': lambda: b.run_system_loglik(s_j, out=out['sys_j']),
        'pem_coupled_system_loglik_f64_dev[system 16 cond]': lambda: b.run_system_loglik(s_sys, out=out['sys']),
        'pem_coupled_system_loglik_f64_dev[stress 8 cond x all kinds]': lambda: b.run_system_loglik(s_stress, out=out['stress']),
        'pem_coupled_loglik_f64_dev[jion 8x32]': lambda: b.run_loglik(jl32, out=out['l32']),
        'pem_coupled_system_loglik_f64_dev[ablation 8 x (32 jion + 9 others)]': lambda: b.run_system_loglik(s_abl, out=out['abl']),
    }
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in runs.values():                                       # warm-up: code objects, LDS attribute, occupancy query
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out['loglik'], out['sys_j']))
    times = {k: [] for k in runs}
    for _ in range(a.rounds):                                       # interleaved: each round times every launch once
        for k, fn in runs.items():
            ev0.record()
            for _ in range(a.reps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) * 1e3 / a.reps)
    res = {'n': a.n, 'reps': a.reps, 'rounds': a.rounds, 'jion_only_bit_identical': same,
           'us_per_launch': {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()},
           'system_table': {'n_cond': s_sys.n_cond, 'n_rec': s_sys.n_rec, 'n_node': s_sys.n_node},
           'stress_table': {'n_cond': ne, 'n_rec': s_stress.n_rec},
           'lds_bytes_per_workgroup': lds, 'workgroups_per_cu_by_lds': {k: min(2, 160 * 1024 // v) for k, v in lds.items()}}
    base = res['us_per_launch']['pem_coupled_loglik_f64_dev[jion 8x40]']['median']
    res['ratio_to_jion_launch'] = {k: v['median'] / base for k, v in res['us_per_launch'].items()}
    print(json.dumps(res, indent=1))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(res, indent=1) + '\n')
    assert same, 'j_ion-only system launch differs from pem_coupled_loglik_f64_dev'


if __name__ == '__main__':
    main()
