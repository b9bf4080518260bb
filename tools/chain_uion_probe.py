#!/usr/bin/env python3
"""Time the chain + likelihood launch that carries u_ion (`pem_chain_fields_loglik_f64_dev`), interleaved with device events after a
warm-up past the clock ramp, on the configs[3] box of tools/chain_probe.py:

  (a) the new entry point with u_rank = 0 against its parent `pem_chain_system_loglik_f64_dev`, same tables: both run the same
      kernel, so a difference beyond the interleaved spread would be a dispatch bug;
  (b) the new launch on a table of V_cc + T + j_ion + u_ion records (u_ion: 8 conditions x 20 positions) against what the parent
      could do for the same answer: `pem_chain_system_loglik_f64_dev` on the table with the u_ion records taken out (rows asked for:
      the V_cc row feeds the thruster's coordinate), the thruster's latents by `pem_sparse_predict_f64_dev`, the profile by
      `pem_svd_reconstruct_f64_dev`, then the gather / interpolation / sum in torch.

    python tools/chain_uion_probe.py [--iters 200] [--reps 20] [--rounds 5] [--out FILE]
"""
import argparse
import copy
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

FIXED = {'P_b': 1e-5, 'V_a': 300.0, 'mdot_a': 5e-6, 'a_1': 0.01, 'sigma_cex': 55e-20, 'c4': 1e20, 'c5': 1e16}
VARIED = ('T_e', 'V_vac', 'Pstar', 'P_T', 'c0', 'c1', 'c2', 'c3')


def fields_loglik_rank0(s, t, lik, out):
    """`ChainedSurrogate.run_system_loglik` of a chain WITHOUT u_ion through the new entry point, u_rank = 0"""
    import torch
    from hallthrusterpem_amd import _lib
    from hallthrusterpem_amd.surrogate import FIELDS
    st, _keep = s.stage_tables()
    c = s.compression
    (vlo, vhi), (ilo, ihi) = s.domains
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None                                     # noqa: E731
    n = t.shape[1]
    _lib.check(_lib.load().pem_chain_fields_loglik_f64_dev(
        n, s.n_dim, s.vcc_slot, s.ib0_slot, st, vlo, vhi - vlo, ilo, ihi - ilo, p(t), max(t.stride(0), n), 1, c.rank, FIELDS['j_ion'], c.norm,
        c.scale, p(c.basis), lik.n_cond, lik.n_rec, p(lik.rec), p(lik.span), None, 0.0, 1.0, p(out), None, 0, None, 0,
        2, 0, 0, 0, 1.0, None, 0, None, None, C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[500_000, 30_000])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from hallthrusterpem_amd.chain import ChainedSurrogate
    from hallthrusterpem_amd.likelihood import SystemLikelihood
    lines = []

    def say(*x):
        s = ' '.join(str(v) for v in x)
        print(s, flush=True)
        lines.append(s)

    t0 = time.perf_counter()
    s = ChainedSurrogate(VARIED, FIXED, u_ion=True)
    for it in range(a.iters):
        s.refine_step(num_refine=1000, seed=it + 1)
    st, _ = s.stage_tables()
    say(f'chain: {a.iters} iterations in {time.perf_counter() - t0:.1f} s; stages n_beta {[g.n_beta for g in st]}, n_out {[g.n_out for g in st]}, '
        f'max_active {[g.max_active for g in st]}, max_level {[g.max_level for g in st]}; j_ion rank {s.compression.rank}, '
        f'u_ion rank {s.u_compression.rank}')
    # the same chain without the latents: the thruster table cut to I_B0 and T (what the parent entry point takes)
    state = copy.deepcopy(s.state())
    state['u_ion'] = None
    state['stages'][1]['values'] = {b: np.ascontiguousarray(v[:, :2]) for b, v in state['stages'][1]['values'].items()}
    s0 = ChainedSurrogate.from_state(state, priors=s.priors)

    rng = np.random.default_rng(0)
    na, nz = 40, 20
    alpha, zloc = np.linspace(-1.5, 1.5, na), np.linspace(0.002, 0.078, nz)
    x = lambda ne: np.stack([np.full(ne, FIXED['P_b']), np.full(ne, FIXED['V_a']), np.full(ne, FIXED['mdot_a'])], 1)   # noqa: E731
    data = {'V_cc': {'x': x(4), 'y': rng.uniform(28, 34, 4), 'var_y': np.full(4, 0.25)},
            'T': {'x': x(4), 'y': rng.uniform(0.07, 0.09, 4), 'var_y': np.full(4, 1e-5)},
            'uion': {'x': x(8), 'y': rng.uniform(1e3, 2e4, (8, nz)), 'var_y': rng.uniform(2e2, 1e3, (8, nz)) ** 2, 'loc': zloc},
            'jion': {'x': x(8), 'y': rng.lognormal(0.0, 1.0, (8, na)), 'var_y': rng.uniform(0.3, 1.5, (8, na)) ** 2,
                     'loc': np.stack([np.ones(na), alpha], 1)}}
    lik = SystemLikelihood(data)
    lik_j = SystemLikelihood({k: data[k] for k in ('V_cc', 'T', 'jion')})
    no_u = copy.copy(lik)                                       # the same conditions, the u_ion records taken out of the spans
    no_u.span = lik.span.clone()
    no_u.span[:, 3] = 0
    say(f'table: {lik.n_cond} conditions, {lik.n_rec} records (each block padded to an odd count), {lik.n_node} u_ion nodes; '
        f'without u_ion data: {lik_j.n_cond} conditions, {lik_j.n_rec} records')
    # the torch part of the composition: the u_ion records of condition c as rows of small tables
    span = lik.span.cpu().numpy()
    ucond = [c for c in range(lik.n_cond) if span[c, 3, 1] > 0]
    rows = torch.zeros((lik.n_cond, nz), dtype=torch.int64, device='cuda')
    on = torch.zeros((lik.n_cond, 1), dtype=torch.float64, device='cuda')
    for c in ucond:
        rows[c] = torch.arange(span[c, 3, 0], span[c, 3, 0] + nz)
        on[c] = 1.0
    w_u, y_u, s_u = (lik.rec[:, k][rows] for k in (0, 1, 2))                                  # [n_cond][nz]
    node = lik.node.long()
    lo_i, hi_i = node[0::2], node[1::2]                                                       # one dataset: every condition shares them
    (vlo, vhi) = s.domains[0]
    vw = torch.tensor(vhi - vlo, dtype=torch.float64, device='cuda')

    for n in a.sizes:
        g = torch.Generator(device='cuda')
        g.manual_seed(1)
        t = torch.rand((len(VARIED), n), dtype=torch.float64, device='cuda', generator=g) * 2 - 1
        cond = torch.arange(n, device='cuda') % lik.n_cond
        ll, ll_c, ll_a, ll_b = (torch.empty(n, dtype=torch.float64, device='cuda') for _ in range(4))
        qoi = torch.empty((4 + s0.stages[2].n_out, n), dtype=torch.float64, device='cuda')

        def composition():
            s0.run_system_loglik(t, no_u, out=ll_c, qoi=qoi)
            tv = (2.0 * (qoi[0] - vlo) / vw - 1.0).reshape(1, n)
            lat = s.stages[1].predict(tv)[2:].T.contiguous()
            u = s.u_compression.reconstruct(lat)
            lo, hi = u[:, lo_i], u[:, hi_i]
            z = (y_u[cond] - torch.addcmul(lo, w_u[cond], hi - lo)) * s_u[cond]
            return ll_c + (-0.5 * z * z).sum(dim=1) * on[cond, 0]

        fused = lambda: s.run_system_loglik(t, lik, out=ll)                                   # noqa: E731
        ref = composition()
        fused()
        torch.cuda.synchronize()
        say(f'\nn = {n}: max |fused - composition| / |composition| = {float(((ll - ref).abs() / ref.abs()).max()):.2e}')
        parent = lambda: s0.run_system_loglik(t, lik_j, out=ll_a)                             # noqa: E731
        rank0 = lambda: fields_loglik_rank0(s0, t, lik_j, ll_b)                               # noqa: E731
        parent()
        rank0()
        torch.cuda.synchronize()
        say(f'  (a) u_rank 0 through the new entry point equals the parent bit for bit: {bool(torch.equal(ll_a, ll_b))}')
        for label, variants in (('(a)', {'new, u_rank 0': rank0, 'parent': parent}), ('(b)', {'fused': fused, 'composition': composition})):
            end = time.perf_counter() + 3.0                                                   # past the clock ramp
            while time.perf_counter() < end:
                for f in variants.values():
                    f()
                torch.cuda.synchronize()
            ms = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, f in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / a.reps)
            say(f'  {label} {a.rounds} interleaved rounds x {a.reps} calls, device events; ms per call: median [min, max]')
            for k, v in ms.items():
                say(f'  {k:14s} {np.median(v):8.4f}  [{min(v):.4f}, {max(v):.4f}]  spread {100 * (max(v) - min(v)) / np.median(v):.2f} %')
            first, second = list(ms)
            say(f'  {first} / {second} = {np.median(ms[first]) / np.median(ms[second]):.4f}')
    say(f'device: {torch.cuda.get_device_name()}')
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    sys.exit(main())
