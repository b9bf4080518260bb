#!/usr/bin/env python3
"""Two figures of DESIGN section 2.1 and 4.1 that no test prints, measured on the GPU against the long double reference of
tests/hp_model.py (test infrastructure; the sections `seed5160` and `recurrence` of profiles/model_hp_r01.txt are this tool's output):

  seed5160    sample 8072 of fuzz seed 5160 (a beam one grid step wide, cos_div next to 1): the kernel's and the oracle's cos_div against
              the truth, the derived bounds of both paths, and what tests/parity_rules.py allows there
  recurrence  the recurrence Gaussians of plume_r1_kernel by themselves: single beams without j_cex (widths set, sigma_cex = 0), the error
              of j_ion[k] against the truth in units of 2^-53 beside the derived count N(k)

    python tools/model_hp_probe.py [seed5160] [recurrence]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / 'tests', ROOT / 'tools'):
    sys.path.insert(0, str(p))

import hp_model as hp  # noqa: E402


def seed5160():
    import parity_rules as pr
    from fuzz_parity import wild
    from oracle import oracle_ctypes as oc
    from hallthrusterpem_amd import constants
    from hallthrusterpem_amd.models import pem_v0_coupled
    K = constants.TORR_2_PA
    x = wild(np.random.default_rng(1000 + 5160), 20_000)
    with np.errstate(all='ignore'):
        want = oc.coupled(x, K)
        got = pem_v0_coupled(x)
        red = pem_v0_coupled(x, profile=False)
        terms = oc.plume_terms(*[x[q] for q in ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')], want['I_B0'], K)
        b = pr.plume_bounds(terms, want['I_B0'])
    i = 8072
    xs = hp.take(x, np.array([i]))
    ref = hp.reference(xs, K)
    LD = hp.LD
    truth = ref['cos_div'][0, 0]
    print('sample', i, {q: float(v[i]) for q, v in x.items()})
    print('a1 %.9f a2 %.6f  cos_div(truth) = 1 - %.6e  div_angle(truth) %.9e' % (float(ref['a1'][0]), float(ref['a2'][0]), float(1 - truth), float(ref['div_angle'][0, 0])))
    for name, res in (('oracle', want), ('kernel, profile', got), ('kernel, reduced', red)):
        d = LD(res['div_angle'][i])
        c = np.cos(d)
        # cos through 1 - 2 sin^2(d / 2): exact to long double next to the pole
        c1 = 2 * np.sin(d / 2) ** 2
        t1 = 2 * np.sin(ref['div_angle'][0, 0] / 2) ** 2
        print('%-16s div_angle %.17e   (cos - truth) / truth = %+.3f u   [1 - cos against 1 - truth: %+.3e relative]' % (name, float(d), float((t1 - c1) / truth) / hp.U, float((c1 - t1) / t1)))
    print('kernel - oracle div_angle relative: %.3e' % abs(got['div_angle'][i] / want['div_angle'][i] - 1))
    for pname, path in (('kernel path (recurrence, fold)', hp.PATH_R1), ('oracle path', hp.PATH_ORACLE)):
        bnd = hp.bounds(ref, path)
        print('%s: derived bound on cos_div %.1f u' % (pname, bnd['e_cos'][0, 0] / hp.U))
    print('parity_rules: cos_rel = %.1f u, of which the 1.5 eps u^2 term %.1f u' % (b['cos_rel'][i, 0] / hp.U, (b['cos_rel'][i, 0] - 4 * pr.EPS) / hp.U))          # (cond = 1 here: the TAU part is zero)
    print('ulp of div_angle at this value: %.3e relative' % (np.spacing(want['div_angle'][i]) / want['div_angle'][i]))


def recurrence():
    from hallthrusterpem_amd import constants
    from hallthrusterpem_amd.models import pem_v0_coupled
    K = constants.TORR_2_PA
    x = hp.widths_set()
    sel = np.flatnonzero((x['sigma_cex'] == 0.0) & (x['c1'] == 1.0))
    xs = hp.take(x, sel)
    ref = hp.reference(xs, K)
    bnd = hp.bounds(ref, hp.PATH_R1)
    got = pem_v0_coupled(xs)
    j, b, _, _ = hp.j_bound(ref, bnd, 0)
    with np.errstate(all='ignore'):
        rel = (np.abs(got['j_ion'].astype(hp.LD) - j) / np.abs(j)).astype(np.float64) / hp.U
        rel = np.where(np.isfinite(rel) & (j.astype(np.float64) > 1e-280), rel, 0.0)
        brel = (b / np.abs(j).astype(np.float64)) / hp.U
    N, C = hp.gauss_counts(hp.PATH_R1)
    print(f'{len(sel)} single-beam samples without j_cex, a from {xs["c3"].min():.3f} to {xs["c3"].max():.3f}')
    print('  k   worst error [u]   its bound [u]   N(k)   at a =      exponent t')
    for k in (0, 1, 5, 11, 22, 23, 24, 45, 46, 60, 68, 69, 80, 89, 90):
        i = int(np.argmax(rel[:, k]))
        print(f'{k:3d}   {rel[i, k]:12.2f}   {brel[i, k]:12.1f}   {N[k]:6.0f}   {xs["c3"][i]:.5f}   {float(ref["t1"][i, k]):10.2f}')
    i, k = np.unravel_index(np.argmax(rel), rel.shape)
    print(f'worst of all: {rel[i, k]:.2f} u = {rel[i, k] * hp.U:.2e} at k = {k}, a = {xs["c3"][i]:.5f}, t = {float(ref["t1"][i, k]):.2f}; the bound there {brel[i, k]:.1f} u')
    wide = xs['c3'] >= 0.25
    i, k = np.unravel_index(np.argmax(rel[wide]), rel[wide].shape)
    print(f'beams of 0.25 rad and wider: {rel[wide][i, k]:.2f} u = {rel[wide][i, k] * hp.U:.2e} at k = {k}, a = {xs["c3"][wide][i]:.5f}')
    print(f'j_ion[0] = I_B0 / (r^2 D(a1)) -- the normaliser through three roundings: worst {rel[:, 0].max():.2f} u at a = {xs["c3"][int(np.argmax(rel[:, 0]))]:.5f}')


if __name__ == '__main__':
    for what in (sys.argv[1:] or ['seed5160', 'recurrence']):
        print(f'==== {what} ====')
        {'seed5160': seed5160, 'recurrence': recurrence}[what]()
