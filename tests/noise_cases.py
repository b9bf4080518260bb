"""The cases the scaled marginal (pem_loglik_marginal_scaled_f64_dev) is held on, shared by tests/test_noise_scale_host.py (the
numpy restatement against the long-double reference) and tests/test_noise_scale_kernels.py (the device against it).  TEST
INFRASTRUCTURE.  Seeded, small, generated on demand.

Shapes: K in {1, 3}; M in {1, 63, 64, 65, 256, 257, 513} (one lane, below / at / past a wave, at / past the workgroup's loop,
into its third round and the merge of all four waves); n_cond in {1, 2, 16} with n_groups in {1, 2, 4, 8}; a group that is the
first condition alone and one that is the last alone; one group with count 0.  Values: scales from {1e-3, 0.5, 1, 2, 1e3}, a mix
of -1 columns, the discharge term absent, fixed and scaled, with and without a prior, ld_theta = d and > d."""
import numpy as np

K_VALUES = (1, 3)
M_VALUES = (1, 63, 64, 65, 256, 257, 513)
COND_GROUPS = ((1, 1), (2, 1), (2, 2), (16, 1), (16, 2), (16, 4), (16, 8))
SCALES = (1e-3, 0.5, 1.0, 2.0, 1e3)
DISCHARGE = (4.5, 0.2)
ENDS = {(1, 1): (1,), (2, 1): (2,), (2, 2): (1, 2), (16, 1): (16,), (16, 2): (1, 16), (16, 4): (1, 8, 15, 16),
        (16, 8): (1, 2, 4, 6, 9, 12, 15, 16)}


def _discharge_inputs(rng, shape):
    return rng.uniform(2e-6, 7e-6, shape), 10.0 ** rng.uniform(np.log10(0.00316), -1.0, shape)


def shape_case(E, G, K, M, variant):
    """one case of the shape (K, M, E) with G groups; `variant` (any integer) picks the discharge mode, the prior, the padding of
    theta, which columns are -1 and which group has no record"""
    rng = np.random.default_rng([E, G, K, M, variant])
    ends = ENDS[(E, G)] if not (G == 2 and E == 16 and variant % 2) else (15, 16)
    counts = rng.integers(1, 40, G).astype(np.float64)
    if G >= 2:
        counts[variant % G] = 0.0
    mode = ('absent', 'fixed', 'scaled')[variant % 3]
    n_model = 2
    scaled = rng.random(G) < 0.7
    if variant % 4 == 0:
        scaled[:] = True
    scale_col = np.where(scaled, n_model + np.cumsum(scaled) - 1, -1).astype(np.int32)
    d = n_model + int(scaled.sum()) + (mode == 'scaled')
    discharge_col = d - 1 if mode == 'scaled' else -1
    ld = d + (3 if variant % 2 else 0)
    theta = np.full((K, ld), np.nan)                       # the padding is never read
    theta[:, :n_model] = rng.normal(size=(K, n_model))
    theta[:, n_model:d] = rng.choice(SCALES, size=(K, d - n_model))
    ll = -rng.gamma(2.0, 1.5, size=(K, M, E))
    mdot_a, a_1 = _discharge_inputs(rng, (K, M, E)) if mode != 'absent' else (None, None)
    log_prior = rng.normal(size=K) * 3.0 if (variant // 3) % 2 else None
    return dict(name=f'E{E} G{G} K{K} M{M} v{variant} {mode}', ll=ll, group_end=np.asarray(ends, dtype=np.int32), group_count=counts,
                theta=theta, d=d, scale_col=scale_col, discharge_col=discharge_col, mdot_a=mdot_a, a_1=a_1, log_prior=log_prior)


def shape_cases(E, G):
    """every (K, M) of the shape list for n_cond = E and G groups, the variants running through all modes"""
    v = 0
    for K in K_VALUES:
        for M in M_VALUES:
            yield shape_case(E, G, K, M, v)
            v += 1


def value_cases():
    """non-finite entries and bad scales: (case, rows of `out` that are -inf, rows that are NaN, rows whose likelihood is not finite:
    there ess and chi are NaN); K = 6, M = 65, E = 2, two groups"""
    rng = np.random.default_rng(77)
    K, M, E = 6, 65, 2
    base = dict(group_end=np.asarray([1, 2], dtype=np.int32), group_count=np.asarray([5.0, 9.0]), d=3,
                scale_col=np.asarray([1, 2], dtype=np.int32), discharge_col=-1, mdot_a=None, a_1=None, log_prior=None)
    ll = -rng.gamma(2.0, 1.5, size=(K, M, E))
    ll[0, 7, 1] = -np.inf                                  # one draw at -inf: it drops out
    ll[1] = -np.inf                                        # every draw at -inf: -inf
    ll[2, 64, 0] = np.nan                                  # one NaN: NaN
    ll[3, :, 0] = -np.inf                                  # a whole group at -inf: -inf
    theta = np.ones((K, 3))
    theta[:, 1:] = rng.choice(SCALES, size=(K, 2))
    yield dict(base, name='non-finite sums', ll=ll, theta=theta), [1, 3], [2], [1, 2, 3]
    lp = rng.normal(size=K)
    lp[4] = -np.inf
    yield dict(base, name='non-finite sums and a prior', ll=ll, theta=theta, log_prior=lp), [1, 2, 3, 4], [], [1, 2, 3]
    md, a1 = _discharge_inputs(rng, (K, M, E))
    for bad in (0.0, -2.0, np.inf, -np.inf, np.nan):
        ll = -rng.gamma(2.0, 1.5, size=(K, M, E))
        theta = np.ones((K, 4))
        theta[:, 1:] = rng.choice(SCALES, size=(K, 3))
        theta[1, 1], theta[3, 2], theta[5, 3] = bad, bad, bad         # the first group's, the second's, the discharge term's
        case = dict(base, name=f'scale {bad}', ll=ll, theta=theta, d=4, discharge_col=3, mdot_a=md, a_1=a1)
        yield case, [], [1, 3, 5], [1, 3, 5]
        yield dict(case, name=f'scale {bad} and a prior', log_prior=lp), [1, 3, 4, 5], [], [1, 3, 5]


def at_scale_one(case, through_theta):
    """the case with every scale exactly 1: every column -1 and no table (`through_theta` False), or every column reading a 1.0"""
    G = len(case['group_end'])
    if not through_theta:
        return dict(case, theta=None, d=0, scale_col=np.full(G, -1, dtype=np.int32), discharge_col=-1)
    theta = np.ones((case['ll'].shape[0], G + 2))
    theta[:, 0] = 3.5
    return dict(case, theta=theta, d=G + 2, scale_col=np.arange(1, G + 1, dtype=np.int32),
                discharge_col=G + 1 if case['mdot_a'] is not None else -1)


def reference(case):
    """hp_noise.marginal_scaled_ref of a case"""
    import hp_noise
    return hp_noise.marginal_scaled_ref(case['ll'], case['group_end'], case['group_count'], case['theta'], case['scale_col'],
                                        case['discharge_col'], case['mdot_a'], case['a_1'], *DISCHARGE, case['log_prior'])


def check(case, out, ess=None, chi=None, ref=None):
    """out (and ess, chi [K][G + 1] where given) of a case against the long-double reference under its bounds"""
    import hp_likelihood as hl
    ref = reference(case) if ref is None else ref
    hl.assert_within(out, ref['out'], ref['out_bound'], f"out, {case['name']}")
    if ess is not None:
        hl.assert_within(ess, ref['ess'], ref['ess_bound'], f"ess, {case['name']}")
    if chi is not None:
        hl.assert_within(chi, ref['chi'], ref['chi_bound'], f"chi, {case['name']}")
    return ref
