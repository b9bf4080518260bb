#!/usr/bin/env python3
"""drivers.sobol_sweep(surrogate=chain) -- one pem_chain_sobol_sweep_f64_dev launch per group -- against the composition of the
launches that existed before it, on one GPU (profiles/chain_sobol_r01.txt).

    python tools/chain_sobol_probe.py [n_base] [rounds]

The composition, per group and pressure and per block of the Saltelli design (A, B, A with column j from B): `Design.sample`
(pem_sample_f64_dev), the torch map to the chain's coordinates, `ChainedSurrogate.predict(field=False)` (all three stages: the plume
stage cannot be left out), the one u_ion cell from the latents in torch, torch reductions of the estimator terms.  Both run the study
of V_cc, T and uion over the five default pressures on the same design rows; the two are timed interleaved, host clock around a
device synchronise, and their indices are compared.
"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'examples'))

QOIS = ('V_cc', 'T', 'uion')


def composition(chain, n_base, pressures, seed, l_ch=0.025):
    """{qoi: {'S1', 'ST': (P, d) tensors}} of the study through `chain`, composed from the launches of the parent commit"""
    import torch
    from hallthrusterpem_amd import sampling
    from hallthrusterpem_amd import sobol as study
    from hallthrusterpem_amd.models.coupled import COUPLED_INPUTS
    dev = chain.device
    cell, _ = study.uion_node(l_ch, chain.uion_grid)
    cu = chain.u_compression
    ub = cu.basis[cell].contiguous()[:, None]
    n_plume = chain.stages[2].n_out
    n_p = len(pressures)
    res = {}
    for g in study.SURROGATE_GROUPS:
        gid = study.GROUPS.index(g)
        names = study.GROUP_INPUTS[g]
        sm = study.surrogate_sweep_map(chain.varied, chain.fixed, chain.priors, pressures, g, True, study.GROUP_QOIS[g])
        rows = torch.as_tensor(sm.rows.astype(np.int64), device=dev)
        is_log = torch.as_tensor(sm.is_log.astype(bool), device=dev)[:, None]
        ca, cw = torch.as_tensor(sm.a, device=dev)[:, None], torch.as_tensor(sm.w, device=dev)[:, None]
        nq = len(study.GROUP_QOIS[g])
        s1 = torch.empty((n_p, len(names), nq), dtype=torch.float64, device=dev)
        st = torch.empty_like(s1)

        def evaluate(design, swap):
            x = design.sample(n_base, device=dev, swap_dim=swap).index_select(0, rows)
            u = torch.where(is_log, torch.log10(x), x)
            out, _ = chain.predict(2.0 * (u - ca) / cw - 1.0, field=False)
            if g == 'Cathode':
                return out[0:1]
            return torch.stack([out[2], (out[4 + n_plume:] * ub).sum(dim=0) / cu.scale])
        for p, pres in enumerate(pressures):
            design = sampling.Design(priors=study.sweep_priors(pres, g), seed=seed, stream=study.row_stream(gid, n_p, p, 0, 0))
            fa, fb = evaluate(design, -1), evaluate(design, -2)
            f = torch.cat([fa, fb], dim=1)
            var = (f * f).mean(dim=1) - f.mean(dim=1) ** 2
            for j, k in enumerate(names):
                fab = evaluate(design, COUPLED_INPUTS.index(k))
                s1[p, j] = (fb * (fab - fa)).mean(dim=1) / var
                st[p, j] = ((fa - fab) ** 2).mean(dim=1) / (2 * var)
        for k, q in enumerate(study.GROUP_QOIS[g]):
            res[q] = {'S1': s1[..., k], 'ST': st[..., k]}
    return res


def main(n_base=100_000, rounds=20):
    import torch
    from hallthrusterpem_amd import drivers
    from hallthrusterpem_amd import sobol as study
    from sobol_sweep import train_chain
    t0 = time.perf_counter()
    chain = train_chain(48)
    torch.cuda.synchronize()
    st, _ = chain.stage_tables()
    print(f'chain: 48 refinements in {time.perf_counter() - t0:.1f} s; stages n_beta {[t.n_beta for t in st]}, n_out {[t.n_out for t in st]}, '
          f'max_active {[t.max_active for t in st]}, max_level {[t.max_level for t in st]}; u_ion rank {chain.u_compression.rank}')
    pb = study.DEFAULT_PRESSURES
    fused = lambda: drivers.sobol_sweep(n_base, qois=QOIS, seed=0, surrogate=chain)                      # noqa: E731
    comp = lambda: composition(chain, n_base, pb, 0)                                                    # noqa: E731
    a, b = fused(), comp()
    torch.cuda.synchronize()
    for q in QOIS:
        d = max(float((a[q][k] - b[q][k]).abs().max()) for k in ('S1', 'ST'))
        print(f'  {q}: largest |index (fused) - index (composition)| = {d:.2e}')
    times = {'fused': [], 'composition': []}
    for _ in range(3):                                                  # warm-up: both, interleaved
        fused()
        comp()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in (('fused', fused), ('composition', comp)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    print(f'n_base = {n_base}, {len(pb)} pressures, V_cc + T + uion ({n_base * len(pb) * 13} surrogate evaluations); {rounds} interleaved calls '
          f'after 3 warm-up calls, host clock around a device synchronise; ms per call: median [min, max]')
    med = {}
    for name, t in times.items():
        med[name] = float(np.median(t))
        print(f'  {name:12s} {med[name]:9.3f}  [{min(t):.3f}, {max(t):.3f}]')
    print(f"  fused / composition = {med['fused'] / med['composition']:.4f}")
    print('device:', torch.cuda.get_device_name(0))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100_000, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
