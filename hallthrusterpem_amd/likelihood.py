"""Gaussian log-likelihood of measured ion current density given plume-model profiles, marginalised over nuisance
samples -- the `jion` branch of `spt100_log_likelihood` (scripts/pem_v0/mcmc.py:57-106).

Layout as in the reference: profiles of shape (..., M, Ne, 91) -- M nuisance draws for each of Ne experimental
conditions -- give `log p(data | theta) = logsumexp_M( sum_{e, a} -0.5 ((y_ea - J(|alpha_ea|)) / std_ea)^2 )`
(the reference also drops the constant terms, mcmc.py:66-69).  The per-sample sums run in one HIP pass over the
profiles (csrc/pem_likelihood.hip); the sum over conditions and the log-sum-exp over M are O(n) torch reductions.
The reference scripts are stale and untested: parity unpinned.

`SystemLikelihood` is the measurement table of the other quantities of the reference's `System` calibration as well -- cathode
coupling voltage, thrust, ion velocity -- for the fused launch `pem_coupled_system_loglik_f64_dev` (mcmc.py:28-45,57-104); with
`sweep_radii` the current densities may be measured at several sweep radii (`pem_coupled_system_loglik_radii_f64_dev`).
"""
import ctypes as C

import numpy as np

from . import _lib

GRID_STEP = (np.pi / 2) / 90.0


class JionLikelihood:
    def __init__(self, alpha, y, std, device=None):
        """alpha, y, std: (Ne, Na) measurement angles (rad, |alpha| <= pi/2; the plume is mirror-symmetric),
        current densities and standard deviations."""
        import torch
        alpha = np.abs(np.atleast_2d(np.asarray(alpha, dtype=np.float64)))
        if alpha.max() > np.pi / 2 + 1e-12:
            raise ValueError('measurement angles beyond 90 degrees are outside the model sweep (plume.py:53)')
        pos = np.minimum(alpha / GRID_STEP, 90.0)
        k = np.minimum(np.floor(pos).astype(np.int32), 89)
        w = pos - k
        self.n_cond, self.n_ang = alpha.shape
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        f = lambda a: torch.as_tensor(np.array(np.broadcast_to(a, alpha.shape)), device=dev)   # noqa: E731
        self.kidx, self.weight = f(k), f(w)
        self.y = f(np.asarray(y, dtype=np.float64))
        self.inv_std = f(1.0 / np.asarray(std, dtype=np.float64))
        self.device = dev

    def per_sample(self, j_ion):
        """j_ion: (..., 91) CUDA tensor whose flattened sample index i belongs to condition i mod Ne -> (...,) sums."""
        import torch
        flat = j_ion.double().contiguous().reshape(-1, _lib.NANGLE)
        out = torch.empty(flat.shape[0], dtype=torch.float64, device=flat.device)
        p = lambda t: C.c_void_p(t.data_ptr())                                                              # noqa: E731
        with torch.cuda.device(flat.device):
            _lib.check(_lib.load().pem_jion_loglik_f64_dev(
                flat.shape[0], self.n_cond, self.n_ang, p(self.kidx), p(self.weight), p(self.y), p(self.inv_std),
                p(flat), p(out), C.c_void_p(torch.cuda.current_stream(flat.device).cuda_stream)))
        return out.reshape(j_ion.shape[:-1])

    def log_likelihood(self, j_ion):
        """j_ion: (..., M, Ne, 91) -> (...,) marginal log-likelihood (log-sum-exp over the M nuisance draws)."""
        import torch
        ll = self.per_sample(j_ion).sum(dim=-1)             # (..., M): all conditions of one draw
        return torch.logsumexp(ll, dim=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# Several measured quantities at once: the `System` calibration of the reference (scripts/pem_v0/mcmc.py:28-45,57-104)
# ---------------------------------------------------------------------------------------------------------------------------
QOIS = ('V_cc', 'T', 'uion', 'jion')
QOI_MAP = {'Cathode': ('V_cc',), 'Thruster': ('T', 'uion'), 'Plume': ('jion',), 'System': QOIS}     # mcmc.py:30
UION_GRID = (0.0, 0.08, 200)
_KIND = {'jion': _lib.SYS_JION, 'V_cc': _lib.SYS_VCC, 'T': _lib.SYS_T, 'uion': _lib.SYS_UION}


class SystemLikelihood:
    """Measurement table of the fused multi-QoI likelihood (`pem_coupled_system_loglik_f64_dev`, run by
    `batch.CoupledBatch.run_system_loglik`): each quantity from its own dataset at its own operating conditions, compared
    with its output of the coupled model -- the clipped cathode coupling voltage `V_cc`, the thruster test double's thrust
    `T`, the ion velocity `uion` interpolated at measured axial positions and the ion current density `jion` at measured
    angles (mcmc.py:57-98).  The reference's driver layer is stale and third-party (surrogate, pem_core datasets): parity
    UNPINNED; the likelihood is held to the oracle + numpy (tests/test_system_likelihood.py).

    :param data: `{qoi: {'x': (Ne, 3) rows of P_b [Torr], V_a [V], mdot_a [kg/s], 'y': ..., 'var_y': ..., 'loc': ...}}` as
                 the reference's DATA, std = sqrt(var_y) (mcmc.py:80).  `y` / `var_y` are (Ne,) for 'V_cc' and 'T';
                 (Ne, Nz) for 'uion' with `loc` the (Nz,) axial positions [m] inside the u_ion grid; (Ne, Na) for 'jion'
                 with `loc` the (Na, 2) rows (r, alpha) of the sweep, every r equal to `sweep_radius` and |alpha| <= pi/2.
    :param sweep_radius: the plume's sweep radius [m] (the j_ion model is evaluated there); default 1.0.  Given together with
                 `sweep_radii` it must equal their last radius.
    :param sweep_radii: None, or 2 .. 8 strictly ascending positive sweep radii [m] for a probe sweep taken at several distances
                 (the reference's data schema gives ion current density the coordinates (r, theta): hallmd/data.py).  Every r of the
                 j_ion `loc` must then equal one of them exactly; a j_ion record carries k | (ridx << 8), and the table is evaluated
                 by `pem_coupled_system_loglik_radii_f64_dev` / `_predict_radii_` -- one model evaluation per sample whatever the
                 number of radii.  `sweep_radius` is then the last (largest) radius, the one div_angle and T_c refer to
                 (`data.pem_to_xarray`'s convention).  One radius is the scalar path.  `sweep_radii` (a tuple) is always set.
    :param uion_grid: (z0, z1, num_cells) of the u_ion profile: z_c = z0 + (z1 - z0) c / (num_cells - 1).  The default
                 (0.0, 0.08, 200) is the grid `models.thruster` uses at the default fidelity (2, 2): num_cells = 50 (f0 + 2)
                 on domain [0, 0.08] (thruster.py:99-107).
    :param qois: a component name of QOI_MAP ('Cathode', 'Thruster', 'Plume', 'System') or a list of QoIs; None = every QoI
                 of `data`, in the order of QOIS.  Conditions are concatenated in this order, as XE_ARRAY (mcmc.py:36-45):
                 sample i of a batch belongs to condition i mod n_cond.
    The record table: one record per measurement (j_ion {w, y, 1/std, k} on the 91-point angle grid, exactly
    `JionLikelihood`'s; u_ion {w, y, 1/std, p} between the nodes node[p], node[p+1]; V_cc / T {0, y, 1/std, 0}), grouped per
    condition, each condition's block padded to an odd number of records (its LDS reads spread over the banks).
    """

    def __init__(self, data, sweep_radius: float | None = None, sweep_radii=None, uion_grid=UION_GRID, qois=None, device=None):
        import torch
        if sweep_radii is not None:
            radii = np.asarray(sweep_radii, dtype=np.float64).reshape(-1)
            limit = _lib.FUSED_SYSTEM_MAX_RADII
            if not 1 <= radii.size <= limit:
                raise ValueError(f'sweep_radii takes 1 .. PEM_FUSED_SYSTEM_MAX_RADII = {limit} radii, got {radii.size}')
            if not np.all(np.isfinite(radii) & (radii > 0.0)):
                raise ValueError(f'sweep_radii must be finite and positive, got {tuple(radii)}')
            if not np.all(np.diff(radii) > 0.0):
                raise ValueError(f'sweep_radii must be strictly ascending, got {tuple(radii)}')
            if sweep_radius is not None and float(sweep_radius) != radii[-1]:
                raise ValueError(f'sweep_radius = {sweep_radius} conflicts with sweep_radii = {tuple(radii)}: with several radii the '
                                 f'scalar is their last one (leave it out)')
            sweep_radius = radii[-1]
        elif sweep_radius is None:
            sweep_radius = 1.0
        if qois is None:
            unknown = [q for q in data if q not in QOIS]
            if unknown:
                raise KeyError(f'unknown QoI {unknown[0]!r}: the measured quantities are {QOIS}')
            qois = tuple(q for q in QOIS if q in data)
        elif isinstance(qois, str):
            if qois not in QOI_MAP:
                raise KeyError(f'unknown component {qois!r}: one of {tuple(QOI_MAP)} or a list of {QOIS}')
            qois = QOI_MAP[qois]
        qois = tuple(qois)
        for q in qois:
            if q not in QOIS:
                raise KeyError(f'unknown QoI {q!r}: the measured quantities are {QOIS}')
            if q not in data:
                raise KeyError(f'no dataset for QoI {q!r}')
        if not qois or len(set(qois)) != len(qois):
            raise ValueError(f'a non-empty list of distinct QoIs is needed, got {qois}')
        self.qois = qois
        self.component = next((k for k, v in QOI_MAP.items() if v == qois), None)
        self.use_discharge = self.component != 'Cathode'            # mcmc.py:100-101
        self.sweep_radius = float(sweep_radius)
        self.sweep_radii = (self.sweep_radius,) if sweep_radii is None else tuple(float(r) for r in radii)
        z0, z1, ncells = float(uion_grid[0]), float(uion_grid[1]), int(uion_grid[2])
        if not (ncells >= 2 and z1 > z0):
            raise ValueError(f'uion_grid = (z0, z1, num_cells) needs z1 > z0 and num_cells >= 2, got {tuple(uion_grid)}')
        self.uion_grid = (z0, z1, ncells)
        # pass 1, on the host only: every dataset checked and the table's size known before a device is touched
        sets = {q: self._check(q, data[q]) for q in qois}
        sizes = [n + (1 - n % 2) for q in qois for n in [sets[q][1].shape[1] if sets[q][1].ndim == 2 else 1] * sets[q][0].shape[0]]
        n_rec, self.n_cond = sum(sizes), len(sizes)
        limit = _lib.FUSED_SYSTEM_MAX_RECORDS
        if n_rec > limit or self.n_cond > limit:
            raise ValueError(f'the measurement table has {n_rec} records (each condition padded to an odd count) over {self.n_cond} '
                             f'conditions; the fused likelihood stages it in LDS and takes at most '
                             f'PEM_FUSED_SYSTEM_MAX_RECORDS = {limit} of each')
        self.device = dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

        # pass 2: records {w, y, 1/std, bits} per condition, conditions in the order of `qois` (mcmc.py:36-45)
        ops, blocks, node, self.conditions = [], [], [], {}
        span = np.zeros((self.n_cond, 4, 2), dtype=np.int32)
        first = 0
        for q in qois:
            x, y, inv_std, loc = sets[q]
            ne = x.shape[0]
            if q in ('V_cc', 'T'):
                w, bits = np.zeros((1,)), np.zeros((1,), dtype=np.int64)
            elif q == 'jion':
                pos = np.minimum(np.abs(loc[:, 1]) / GRID_STEP, 90.0)       # JionLikelihood's (k, w), bit for bit
                k = np.minimum(np.floor(pos).astype(np.int32), 89)
                w, bits = pos - k, k.astype(np.int64)
                if len(self.sweep_radii) > 1:                               # the index of the record's radius above the angle index
                    bits = bits | (np.searchsorted(self.sweep_radii, loc[:, 0]).astype(np.int64) << 8)
            else:   # uion: between the nodes of the kernels' own grid doubles
                z = self._uion_nodes(z0, z1, ncells)
                k = np.clip(np.searchsorted(z, loc, side='right') - 1, 0, ncells - 2)
                w = (loc - z[k]) / (z[k + 1] - z[k])
                bits = len(node) + 2 * np.arange(loc.size, dtype=np.int64)
                node += [v for kk in k for v in (int(kk), int(kk) + 1)]
            self.conditions[q] = slice(len(ops), len(ops) + ne)
            for e in range(ne):
                recs = np.zeros((y.shape[1] + (1 - y.shape[1] % 2), 4))    # odd stride between conditions (LDS banks)
                na = y.shape[1]
                recs[:na, 0], recs[:na, 1], recs[:na, 2] = w, y[e], inv_std[e]
                recs[:na, 3] = np.ascontiguousarray(np.broadcast_to(bits, (na,))).view(np.float64)
                span[len(ops), _KIND[q]] = (first, na)
                first += recs.shape[0]
                ops.append(x[e])
                blocks.append(recs)
        self.operating = np.stack(ops)
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)                                      # noqa: E731
        self.n_rec, self.n_node = n_rec, len(node)
        self.rec = f(np.concatenate(blocks))
        self.span = f(span)
        self.node_host = np.asarray(node if node else [0, 0], dtype=np.int32)      # (an entry point that checks the table reads this copy)
        self.node = f(self.node_host)
        self.data = {q: data[q] for q in qois}

    def _check(self, q, d):
        """(x (Ne, 3), y (Ne, n), 1/std (Ne, n), loc) of one dataset, n = 1 for the scalar QoIs; refuses what does not fit."""
        if not isinstance(d, dict) or 'x' not in d or 'y' not in d or 'var_y' not in d:
            raise ValueError(f"{q}: a dataset is a dict with 'x', 'y', 'var_y' (and 'loc' for uion / jion)")
        x = np.asarray(d['x'], dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != 3 or x.shape[0] < 1:
            raise ValueError(f"{q}: 'x' must be (Ne, 3) rows of P_b, V_a, mdot_a, got shape {x.shape}")
        ne = x.shape[0]
        y, var = np.asarray(d['y'], dtype=np.float64), np.asarray(d['var_y'], dtype=np.float64)
        loc = None
        if q in ('V_cc', 'T'):
            want = (ne,)
        elif q == 'jion':
            loc = np.asarray(d.get('loc'), dtype=np.float64)
            if loc.ndim != 2 or loc.shape[1] != 2 or loc.shape[0] < 1:
                raise ValueError(f"jion: 'loc' must be (Na, 2) rows of (r, alpha), got shape {loc.shape}")
            if len(self.sweep_radii) > 1:
                if not np.all(np.isin(loc[:, 0], self.sweep_radii)):
                    raise ValueError(f'jion: every radius of loc must equal one of sweep_radii = {self.sweep_radii} exactly, got '
                                     f'{np.unique(loc[:, 0])}')
            elif not np.all(loc[:, 0] == self.sweep_radius):
                raise ValueError(f'jion: every radius of loc must equal sweep_radius = {self.sweep_radius} (one sweep radius '
                                 f'per dataset), got {np.unique(loc[:, 0])}')
            if not np.all(np.abs(loc[:, 1]) <= np.pi / 2 + 1e-12):
                raise ValueError('jion: measurement angles beyond 90 degrees are outside the model sweep (plume.py:53)')
            want = (ne, loc.shape[0])
        else:
            loc = np.asarray(d.get('loc'), dtype=np.float64)
            z0, z1, _ = self.uion_grid
            if loc.ndim != 1 or loc.size < 1:
                raise ValueError(f"uion: 'loc' must be the (Nz,) axial positions, got shape {loc.shape}")
            if not np.all((loc >= z0) & (loc <= z1)):
                raise ValueError(f'uion: axial positions outside the u_ion grid [{z0}, {z1}] (interp1d does not extrapolate): '
                                 f'{loc[(loc < z0) | (loc > z1) | np.isnan(loc)]}')
            want = (ne, loc.size)
        if y.shape != want:
            raise ValueError(f"{q}: 'y' must have shape {want} for {ne} operating conditions in 'x', got {y.shape}")
        if var.shape != want:
            raise ValueError(f"{q}: 'var_y' must have shape {want}, got {var.shape}")
        inv_std = 1.0 / np.sqrt(var)                                   # std = sqrt(var_y), mcmc.py:80
        return x, y.reshape(ne, -1), inv_std.reshape(ne, -1), loc

    def _uion_nodes(self, z0, z1, ncells):
        """The grid doubles of the kernels (pem_thruster_uion_f64_dev's z), so that (k, w) are taken from the nodes the
        likelihood launch interpolates between."""
        import torch
        z = torch.empty(ncells, dtype=torch.float64, device=self.device)
        one = torch.ones(1, dtype=torch.float64, device=self.device)
        u = torch.empty(ncells, dtype=torch.float64, device=self.device)
        p = lambda t: C.c_void_p(t.data_ptr())                                                              # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_thruster_uion_f64_dev(1, p(one), z0, z1, ncells, p(z), p(u),
                                                             C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return z.cpu().numpy()
