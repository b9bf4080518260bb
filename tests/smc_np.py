"""numpy restatement of the two launches of csrc/pem_smc.hip (`pem_smc_stage_f64_dev`, `pem_smc_move_f64_dev`; the rules are in
include/pem_hip.h): the same Philox counters, the cumulative weights in the stated order, the same IEEE operations in the same
order for the ancestors, the gather, the proposals, the counters and the history.  What goes through exp / log / normcdfinv or
through a sum whose order the header leaves open has a last bit of its own on the device, so `stage` accepts the device's
beta_next, w (the un-normalised weights at beta'), L and normals, and `move` its normals and decisions; with those given every
other state word compares bit for bit.  `run` drives two numpy callables through a whole run.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import dram_np
from oracle import sampler_np as snp

RESAMPLE, Z, U = 0x534D0000, 0x534D0001, 0x534D0002
ST, WAVE, BISECTIONS = 1024, 64, 52
_U = np.uint64
_M = _U(0xFFFFFFFF)


def _keys(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def new_state(theta, loglik, logprior, history_len=64):
    """the state words as the caller hands them to the first stage launch"""
    theta = np.array(theta, dtype=np.float64)
    R, N, d = theta.shape
    z = lambda *s, dt=np.float64: np.zeros(s, dtype=dt)                                              # noqa: E731
    return dict(theta=theta, loglik=np.array(loglik, dtype=np.float64).reshape(R, N),
                logprior=np.array(logprior, dtype=np.float64).reshape(R, N), beta=z(R), log_evidence=z(R), stage=z(R, dt=np.int64),
                L=z(R, d, d), prop=z(R, N, d), accept_count=z(R, N, dt=np.uint32), accepted=z(R, dt=np.int64),
                flags=z(R, dt=np.uint32), moves_active=z(R, dt=np.uint32), hist_beta=z(R, history_len), hist_ess=z(R, history_len),
                hist_accept=z(R, history_len), hist_dlogz=z(R, history_len))


def shifted(loglik):
    """(l - l_max with -inf where l is not finite, l_max, finite mask) of one population; l_max None when nothing is finite"""
    fin = np.isfinite(loglik)
    if not fin.any():
        return None, None, fin
    lmax = loglik[fin].max()
    with np.errstate(all='ignore'):
        return np.where(fin, loglik - lmax, -np.inf), lmax, fin


def weight_argument(dl, b0, b):
    """(b - beta) (l - l_max), what the device takes the exp of (0 stands in where the weight is 0 by rule)"""
    with np.errstate(all='ignore'):
        return np.where(dl == -np.inf, 0.0, (b - b0) * dl)


def weights(dl, b0, b):
    return np.where(dl == -np.inf, 0.0, np.exp(weight_argument(dl, b0, b)))


def ess_of(w):
    return w.sum() ** 2 / (w * w).sum()


def next_beta(dl, b0, tau):
    """step 1 of the stage launch with numpy's exp and sums"""
    tau_n = tau * float(dl.size)
    if ess_of(weights(dl, b0, 1.0)) >= tau_n:
        return 1.0
    lo, hi = b0, 1.0
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        if ess_of(weights(dl, b0, mid)) >= tau_n:
            lo = mid
        else:
            hi = mid
    return lo if lo > b0 else hi


def cumulative(w):
    """C in the header's order: thread t of 1024 sums its P = ceil(N / 1024) weights in particle order, the threads of a wave of
    64 chain their totals from 0, the 16 waves chain theirs from 0, and C_i = W_wave + (O_thread + c_i)"""
    N = w.size
    P = -(-N // ST)
    pad = np.zeros(ST * P)
    pad[:N] = w
    c = np.cumsum(pad.reshape(ST, P), axis=1)
    incl = np.cumsum(c[:, -1].reshape(ST // WAVE, WAVE), axis=1)
    O = np.concatenate([np.zeros((ST // WAVE, 1)), incl[:, :-1]], axis=1)
    wave_incl = np.cumsum(incl[:, -1])
    Woff = np.concatenate([[0.0], wave_incl[:-1]])
    C = Woff[:, None, None] + (O[:, :, None] + c.reshape(ST // WAVE, WAVE, P))
    return C.reshape(-1)[:N]


def resample_uniform(seed, r, stage_number):
    k0, k1 = _keys(seed)
    x = snp.philox4x32_10(r, stage_number & 0xFFFFFFFF, RESAMPLE, 0, k0, k1)
    return float(snp.u53(x[0], x[1]))


def ancestors(w, u):
    N = w.size
    C = cumulative(w)
    t = ((np.arange(N, dtype=np.float64) + u) / float(N)) * C[N - 1]
    last = int(np.nonzero(w > 0.0)[0].max())
    return np.minimum(np.searchsorted(C, t, side='right'), last), C


def moments(w, theta):
    """normalised weights, weighted mean and covariance of one population (numpy's own sums)"""
    W = w / w.sum()
    mean = W @ theta
    y = theta - mean
    return W, mean, (W[:, None] * y).T @ y


def draw_normals(seed, first, N, d, word):
    """(N, d) normals of particles first ... first + N - 1 (numbered over all populations) under counter word `word`"""
    from scipy.special import ndtri
    k0, k1 = _keys(seed)
    gp = (np.arange(N, dtype=_U) + _U(first)) & _M
    cols = []
    for j in range(d):
        r = snp.philox4x32_10(gp, int(word) & 0xFFFFFFFF, Z, j // 2, k0, k1)
        cols.append(ndtri(dram_np.u_open(r[0], r[1]) if j % 2 == 0 else dram_np.u_open(r[2], r[3])))
    return np.stack(cols, axis=1)


def propose(theta, L, z):
    """y_j = x_j + sum_{i <= j} L_ji z_i for the (N, d) particles of one population, i ascending"""
    N, d = theta.shape
    out = np.empty((N, d))
    for j in range(d):
        t = np.zeros(N)
        for i in range(j + 1):
            t = t + L[j, i] * z[:, i]
        out[:, j] = theta[:, j] + t
    return out


def stage(st, seed, tau, scale, eps, n_mcmc, beta_next=None, w=None, L=None, normals=None):
    """One stage launch.  beta_next (R,), w (R, N), L (R, d, d), normals (R, N, d): the device's, in place of this file's own
    (entries of populations the launch does not advance are not looked at).  Returns (new state, record): per population None, or
    a dict of what the launch used (b0, lmax, dl, w, W, anc, u, mean, cov, z, ess, inc)."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    R, N, d = out['theta'].shape
    H = out['hist_beta'].shape[1]
    recs = []
    for r in range(R):
        b0, s0 = float(st['beta'][r]), int(st['stage'][r])
        if st['moves_active'][r]:
            acc = int(st['accept_count'][r].astype(np.int64).sum())
            out['accepted'][r] = acc
            if 1 <= s0 <= H:
                out['hist_accept'][r, s0 - 1] = float(acc) / (float(N) * float(n_mcmc))
        if not b0 < 1.0:
            out['moves_active'][r] = 0
            recs.append(None)
            continue
        dl, lmax, _ = shifted(st['loglik'][r])
        if dl is None:
            out['flags'][r] |= 2
            out['moves_active'][r] = 0
            recs.append(None)
            continue
        b1 = float(next_beta(dl, b0, tau) if beta_next is None else beta_next[r])
        wr = weights(dl, b0, b1) if w is None else np.asarray(w[r], dtype=np.float64)
        ess = ess_of(wr)
        inc = np.log(wr.sum() / float(N)) + (b1 - b0) * lmax
        W, mean, cov = moments(wr, st['theta'][r])
        if L is None:
            A, failed = dram_np.cholesky(((scale * scale) * cov + eps * np.eye(d))[None], st['L'][r][None])
            out['L'][r] = A[0]
            if failed[0]:
                out['flags'][r] |= 1
        else:                                        # the device's factor; it kept the old one and raised bit 0 on a bad pivot
            out['L'][r] = L[r]
        u = resample_uniform(seed, r, s0 + 1)
        anc, _ = ancestors(wr, u)
        out['theta'][r] = st['theta'][r][anc]
        out['loglik'][r] = st['loglik'][r][anc]
        out['logprior'][r] = st['logprior'][r][anc]
        out['accept_count'][r] = 0
        if s0 < H:
            out['hist_beta'][r, s0], out['hist_ess'][r, s0], out['hist_dlogz'][r, s0] = b1, ess, inc
        out['beta'][r] = b1
        out['log_evidence'][r] = st['log_evidence'][r] + inc
        out['stage'][r] = s0 + 1
        out['moves_active'][r] = 1
        z = draw_normals(seed, r * N, N, d, (s0 + 1) * n_mcmc + 1) if normals is None else np.asarray(normals[r])
        out['prop'][r] = propose(out['theta'][r], out['L'][r], z)
        recs.append(dict(b0=b0, b1=b1, lmax=lmax, dl=dl, w=wr, W=W, anc=anc, u=u, mean=mean, cov=cov, z=z, ess=ess, inc=inc))
    return out, recs


def move(st, prop_loglik, prop_logprior, seed, n_mcmc, move, propose_next=True, normals=None, decisions=None):
    """One move launch: resolves proposal `move` (1 ... n_mcmc) of the stage and, with propose_next, draws proposal move + 1.
    normals (R, N, d) / decisions (R, N) bool: the device's, in place of this file's own.  Returns (new state, record): u, lhs =
    log(u), rhs, acc as this file decides them (R, N), and z (R, N, d) (None without propose_next)."""
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    R, N, d = out['theta'].shape
    k0, k1 = _keys(seed)
    pl, pp = np.asarray(prop_loglik).reshape(R, N), np.asarray(prop_logprior).reshape(R, N)
    active = np.asarray(st['moves_active']).astype(bool)
    word = (np.asarray(st['stage'], dtype=np.int64) * n_mcmc + move) & 0xFFFFFFFF
    gp = (np.arange(R * N, dtype=_U) & _M).reshape(R, N)
    x = snp.philox4x32_10(gp, word.astype(_U)[:, None], U, 0, k0, k1)
    u = snp.u53(x[0], x[1])
    with np.errstate(all='ignore'):
        lhs = np.log(u)
        rhs = (pp - st['logprior']) + np.asarray(st['beta'])[:, None] * (pl - st['loglik'])
        own = np.isfinite(pl) & np.isfinite(pp) & (lhs < rhs)
    acc = (own if decisions is None else np.asarray(decisions).astype(bool).reshape(R, N)) & active[:, None]
    out['theta'][acc] = st['prop'][acc]
    out['loglik'][acc] = pl[acc]
    out['logprior'][acc] = pp[acc]
    out['accept_count'] += acc.astype(np.uint32)
    zs = None
    if propose_next:
        zs = np.zeros((R, N, d))
        for r in np.nonzero(active)[0]:
            zs[r] = draw_normals(seed, r * N, N, d, int(word[r]) + 1) if normals is None else np.asarray(normals[r])
            out['prop'][r] = propose(out['theta'][r], out['L'][r], zs[r])
    return out, dict(u=u, lhs=lhs, rhs=rhs, acc=own, z=zs)


def run(loglik, logprior, theta0, seed=0, tau=0.5, n_mcmc=3, scale=None, eps=1e-12, max_stages=200):
    """A whole run of numpy callables on (R N, d) arrays from the prior draws theta0 (R, N, d): stage launches and n_mcmc move
    launches each until every population is at beta = 1, then the stage launch that closes the last stage's acceptance.  Returns
    the final state; its history arrays have max_stages columns."""
    theta0 = np.array(theta0, dtype=np.float64)
    R, N, d = theta0.shape
    scale = 2.38 / np.sqrt(d) if scale is None else scale
    flat = theta0.reshape(R * N, d)
    st = new_state(theta0, loglik(flat), logprior(flat), history_len=max_stages)
    for _ in range(max_stages):
        st, _ = stage(st, seed, tau, scale, eps, n_mcmc)
        if not st['moves_active'].any():
            break
        for m in range(1, n_mcmc + 1):
            flat = st['prop'].reshape(R * N, d)
            st, _ = move(st, loglik(flat), logprior(flat), seed, n_mcmc, m, propose_next=m < n_mcmc)
    else:
        st, _ = stage(st, seed, tau, scale, eps, n_mcmc)
    return st
