#!/usr/bin/env python3
"""What calibration.DeviceSMC costs on the `System` posterior of the README's DRAM row (needs the GPU).

Workload: the `System` table of tools/dram_step_probe.py (16 conditions, 348 records), the six calibrated inputs of
tools/ensemble_probe.py, M = 50 shared nuisance draws, R = 1 population of N = 1024 and of N = 4096 particles from Sobol' draws of
the prior, tau = 0.5, n_mcmc = 3.  Per N, alternating in one process, `--repeats` times each:

  the stage launch alone        device events around one pem_smc_stage_f64_dev launch on the prior draws (beta 0 -> beta'); the state
                                is put back between launches, outside the events
  the move launch alone         replays of a one-node graph of pem_smc_move_f64_dev (it resolves against the same values again and
                                again: the same work)
  one posterior evaluation      replays of a graph of [log_likelihood(prop), log_prior(prop)] on the same N rows
  one stage replay              the graph DeviceSMC replays: [stage launch ; 3 x (evaluation ; move launch)], replayed from the
                                prior draws for as many stages as the run needs, one device synchronise at the end
  a whole run                   DeviceSMC.run() from the prior draws to beta = 1, host clock, with its readbacks of beta

and beside them a `DeviceTemperedEnsemble` step (R = 1, T = 4, K = 32, as tools/tempering_probe.py) on the same table.

    python tools/smc_probe.py [--repeats 3] [--out profiles/smc_r01.txt]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
from dram_step_probe import per_step, system_table                                              # noqa: E402
from hallthrusterpem_amd.calibration import DeviceEnsemble, DeviceSMC, DeviceTemperedEnsemble, SystemPosterior, capture_graph   # noqa: E402

NAMES = ('T_e', 'V_vac', 'P_T', 'a_1', 'c0', 'c3')
M = 50


def replays(graph):
    def run(n):
        for _ in range(n):
            graph.replay()
    return run


class Case:
    """one N: the sampler at its prior draws, with the state saved to come back to"""

    def __init__(self, lik, N, max_stages):
        self.N, self.max_stages = N, max_stages
        self.post = SystemPosterior(NAMES, lik, n_chains=N, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True)
        theta0 = DeviceSMC.prior_draws(NAMES, n_particles=N, seed=2, device=self.post.device)
        self.sm = DeviceSMC(self.post.log_likelihood, self.post.log_prior, theta0, seed=3, device=self.post.device)
        self.sm._prepare(max_stages)
        self.saved = [t.clone() for t in self.sm._state()]
        res = self.run()
        self.stages, self.converged, self.result = int(res.stages[0]), bool(res.converged[0]), res
        sm = self.sm
        flat = sm.prop.view(sm.R * sm.N, sm.d)

        def evaluate():
            sm.prop_loglik.view(-1).copy_(sm.f_lik(flat))
            sm.prop_logprior.view(-1).copy_(sm.f_prior(flat))
        self.restore()
        sm._launch_stage()                           # a state with proposals pending, for the two graphs below
        self.eval_graph = capture_graph(evaluate, sm.device)[0]
        self.move_graph = capture_graph(lambda: sm._launch_move(1, True), sm.device)[0]
        self.restore()

    def restore(self):
        for t, s in zip(self.sm._state(), self.saved):
            t.copy_(s)

    def run(self):
        self.restore()
        return self.sm.run(max_stages=self.max_stages, check_every=4)

    def stage_alone_us(self, n=20):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        out = []
        for _ in range(n):
            self.restore()
            torch.cuda.synchronize()
            ev[0].record()
            self.sm._launch_stage()
            ev[1].record()
            torch.cuda.synchronize()
            out.append(ev[0].elapsed_time(ev[1]) * 1e3)
        self.restore()
        return float(np.median(out))

    def move_alone_us(self, n):
        self.restore()
        self.sm._launch_stage()                      # moves_active, proposals pending and their values: what a move launch meets
        self.eval_graph.replay()
        replays(self.move_graph)(50)
        t = per_step(replays(self.move_graph), n)
        self.restore()
        return t

    def stage_replay_us(self):
        self.restore()
        t = per_step(replays(self.sm._graph), self.stages)
        assert bool((self.sm.beta == 1.0).all()) == self.converged
        return t

    def run_ms(self):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = self.run()
        torch.cuda.synchronize()
        assert int(res.stages[0]) == self.stages
        return (time.perf_counter() - t0) * 1e3


def stage_breakdown(N, d, n=20):
    """the stage launch alone on synthetic values, by difference: a finished population (the launch and its early return), all log
    likelihoods equal (beta' = 1 at once: everything but the 52 halvings), and a spread of log likelihoods (the whole launch)"""
    dev = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(7)
    theta = rng.standard_normal((1, N, d))
    out = {}
    for label, ll in (('whole', -50.0 * rng.random(N) ** 2), ('no bisection', np.zeros(N)), ('finished', np.zeros(N))):
        ll_t, lp_t = torch.as_tensor(ll, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
        sm = DeviceSMC(lambda x: ll_t, lambda x: lp_t, theta, use_graph=False, device=dev)
        sm._prepare(4)
        if label == 'finished':
            sm.beta.fill_(1.0)
        saved = [t.clone() for t in sm._state()]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        t = []
        for _ in range(n + 3):
            for a, b in zip(sm._state(), saved):
                a.copy_(b)
            torch.cuda.synchronize()
            ev[0].record()
            sm._launch_stage()
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]) * 1e3)
        out[label] = float(np.median(t[3:]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--replays', type=int, default=300)
    ap.add_argument('--max-stages', type=int, default=400)
    ap.add_argument('--particles', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'smc_r01.txt'))
    a = ap.parse_args()
    lik = system_table()
    assert lik.n_cond == 16 and lik.n_rec == 348
    cases = {N: Case(lik, N, a.max_stages) for N in a.particles}
    T, K = 4, 32
    post_pt = SystemPosterior(NAMES, lik, n_chains=T * K // 2, n_nuisance=M, seed=1, fresh_nuisance=False, shared_nuisance=True)
    theta0 = np.array([3.0, 30.0, 5e-5, 0.03, 0.5, 0.9])
    pt = DeviceTemperedEnsemble(post_pt.log_likelihood, post_pt.log_prior,
                                DeviceEnsemble.ball(theta0, 0.01 * theta0, K, n_ensembles=T, seed=3), betas=[1.0, 0.5, 0.25, 0.125],
                                seed=2, device=post_pt.device)
    pt.run(200, keep=False)
    times = {}
    add = lambda k, v: times.setdefault(k, []).append(v)                                             # noqa: E731
    for _ in range(a.repeats):
        for N, c in cases.items():
            add(f'N = {N}: pem_smc_stage_f64_dev alone, device events (us)', c.stage_alone_us())
            add(f'N = {N}: pem_smc_move_f64_dev alone, graph replay (us)', c.move_alone_us(a.replays))
            replays(c.eval_graph)(10)
            add(f'N = {N}: log_likelihood + log_prior of {N} rows, graph replay (us)', per_step(replays(c.eval_graph), a.replays))
            add(f'N = {N}: one stage replay, mean over the {c.stages} stages of a run (us)', c.stage_replay_us())
            add(f'N = {N}: a whole run to beta = 1, with readbacks every 4 stages (ms)', c.run_ms())
        add(f'DeviceTemperedEnsemble step, T = {T}, K = {K}, 2 x [log_likelihood, log_prior](64 rows) (us)',
            per_step(lambda n: pt.run(n, keep=False), 1000))
    lines = [f'DeviceSMC on one MI355X ({torch.cuda.get_device_name(0)}), python tools/smc_probe.py, {time.strftime("%Y-%m-%d")}',
             f'Workload: System table of {lik.n_cond} conditions, {lik.n_rec} records; d = {len(NAMES)} calibrated inputs {" ".join(NAMES)}; '
             f'M = {M} shared nuisance draws;',
             "R = 1 population from Sobol' draws of the prior, tau = 0.5, n_mcmc = 3: a stage is 1 stage launch + 3 x (N-row evaluation + "
             'move launch), one graph replay.',
             f'The measurements alternate, {a.repeats} repeats each: median [min, max], repeats', '']
    for k, t in times.items():
        lines.append(f'  {k:88s} {np.median(t):10.1f}  [{min(t):.1f}, {max(t):.1f}]   ' + ' '.join(f'{v:.1f}' for v in t))
    lines.append('')
    for N, c in cases.items():
        r = c.result
        n = c.stages
        evals = N * (1 + 3 * n)
        lines += [f'  N = {N}: {n} stages to beta = 1 (converged {c.converged}, flags {int(r.flags[0])}), {evals} posterior evaluations '
                  f'({evals * M * lik.n_cond} coupled samples), log evidence {r.log_evidence[0]:.3f}',
                  '    beta        ' + ' '.join(f'{v:.3g}' for v in r.betas[0]),
                  '    acceptance  ' + ' '.join(f'{v:.2f}' for v in r.acceptance[0]),
                  f'    ESS / N of the stages but the last: {np.min(r.ess[0, :n - 1]) / N if n > 1 else float("nan"):.6f} ... '
                  f'{np.max(r.ess[0, :n - 1]) / N if n > 1 else float("nan"):.6f}']
    lines += ['', 'The stage launch alone on synthetic values, by difference (us, median of 20 event timings): whole launch / all log '
              "likelihoods equal, so beta' = 1 without the 52 halvings / a finished population, the launch and its early return"]
    for N in a.particles:
        for d in (1, 6, 32):
            b = stage_breakdown(N, d)
            lines.append(f'  N = {N:5d} d = {d:2d}:  {b["whole"]:8.1f} / {b["no bisection"]:8.1f} / {b["finished"]:8.1f}')
    text = '\n'.join(lines) + '\n'
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)
    print(json.dumps({k: {'median': float(np.median(t)), 'repeats': t} for k, t in times.items()}))


if __name__ == '__main__':
    main()
