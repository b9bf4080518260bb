"""One surrogate per component, chained through the coupling variables (round 5).

The reference trains a surrogate for each component of the PEM-v0 graph and feeds one component's predicted coupling output to
the next (scripts/pem_v0/pem_v0_SPT-100.yml:4-6,55-63,110-178,215-280; scripts/fit_surr.py:111-160 spends its budget per
component):

    Cathode   P_b, V_a, T_e, V_vac, Pstar, P_T              -> V_cc
    Thruster  V_a, V_cc, mdot_a, a_1                        -> I_B0, T [, u_ion as SVD latents]   (the analytic TEST DOUBLE,
                                                                                  tests/sim_hallthruster.jl)
    Plume     P_b, c0 .. c5, sigma_cex, I_B0                -> div_angle [, j_ion as SVD latents]

Each component is a `surrogate.SparseGridSurrogate` over its own inputs (its hooks: the component's input names, its model, the
linear domain of its coupling input, the coordinate count of the chained launch).  A coupling input's domain is estimated as
fit_surr.py:111's `estimate_bounds=True` asks: the upstream true model at 500 uniform points of its own box, widened by 5 %.
The refinement is amisc's cost-weighted greedy allocation: every iteration scores every component's candidates and activates the
(component, candidate) with the largest indicator / (new nodes x cost share).  The prediction is ONE launch,
`pem_sparse_predict_chain_f64_dev` (csrc/pem_surrogate.hip), or `pem_sparse_predict_chain_fields_f64_dev` when the thruster carries
the ion velocity profile (yml:207-214: svd under norm linear(1.0e-3), trained with the thruster component, train-shim.sh:9-11).
amisc is third-party and absent: parity UNPINNED.
"""
import ctypes as C

import numpy as np

from . import _lib, sampling
from .models.coupled import COUPLED_INPUTS
from .surrogate import FIELDS, SparseGridSurrogate

COMPONENT_INPUTS = (('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T'),
                    ('V_a', 'V_cc', 'mdot_a', 'a_1'),
                    ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex', 'I_B0'))
COMPONENT_OUTPUTS = (('V_cc',), ('I_B0', 'T'), ('div_angle',))
COUPLING = ('V_cc', 'I_B0')            # cathode -> thruster, thruster -> plume
# algorithmic bytes per evaluation of each component's own kernel: the cost model of the allocation,
# normalised so that one evaluation of the whole graph still costs 1
COST_BYTES = (56.0, 96.0, 808.0)
COST_SHARES = tuple(b / sum(COST_BYTES) for b in COST_BYTES)
NUM_BOUNDS = 500                       # upstream evaluations per coupling domain (fit_surr.py:111 estimate_bounds)
CHAIN_OUTPUTS = ('V_cc', 'I_B0', 'T', 'div_angle', 'T_c')


def _dev(inputs, keys, device):
    import torch
    return {k: torch.as_tensor(np.asarray(inputs[k], dtype=np.float64), device=device) for k in keys}


def cathode_model(device):
    from .models.cathode import cathode_coupling

    def run(inputs, n):                                   # pem_cathode_f64_dev -> [n][1]
        return cathode_coupling(_dev(inputs, COMPONENT_INPUTS[0], device))['V_cc'].reshape(n, 1)
    return run


def thruster_model(device, compression=None, grid=None):
    from .models.thruster import thruster_analytic

    def run(inputs, n):                                   # pem_thruster_f64_dev [+ _uion_, pem_svd_compress_f64_dev] -> [n][I_B0, T, latents]
        import torch
        x = _dev(inputs, COMPONENT_INPUTS[1], device)
        o = thruster_analytic(x) if compression is None else thruster_analytic(x, num_cells=grid[2], domain=grid[:2])
        y = torch.stack([o['I_B0'].reshape(n), o['T'].reshape(n)], dim=1)
        return y if compression is None else torch.cat([y, compression.compress(o['u_ion'].reshape(n, grid[2]))], dim=1)
    return run


def _compression_state(comp):
    if comp is None:
        return None
    return {'rank': comp.rank, 'basis': comp.basis.cpu().numpy(), 'relative_error': getattr(comp, 'relative_error', None),
            'norm': comp.norm, 'scale': comp.scale, 'reconstruction_tol': comp.reconstruction_tol}


def _compression_from_state(st, norm='log10'):
    """a fitted SVDCompression from `_compression_state`'s dict; a state written before the norm was kept is the log10 map of j_ion"""
    import torch
    from .compression import SVDCompression
    if st is None:
        return None
    name = {0: 'none', 1: 'log10', 2: 'linear'}[st['norm']] if 'norm' in st else norm
    comp = SVDCompression(norm=name, scale=st.get('scale', 1.0), reconstruction_tol=st.get('reconstruction_tol', 0.01), rank=st['rank'])
    comp.basis = torch.from_numpy(np.asarray(st['basis'])).cuda()
    comp.relative_error = st['relative_error']
    return comp


def plume_run(inputs, n, device):
    """pem_plume_f64_dev at one sweep radius (1 m, yml:218): (div_angle (n,), j_ion (n, 91), invalid (n,) bool)"""
    import torch
    from . import _marshal as m, constants
    x = _dev(inputs, COMPONENT_INPUTS[2], device)
    div = torch.empty(n, dtype=torch.float64, device=device)
    j = torch.empty((n, _lib.NANGLE), dtype=torch.float64, device=device)
    bad = torch.empty(n, dtype=torch.uint8, device=device)
    radius = np.ones(1)                                   # a HOST array read by the call: it must outlive it
    with torch.cuda.device(device):
        _lib.check(_lib.load().pem_plume_f64_dev(n, 1, m.np_ptr(radius), constants.TORR_2_PA, *[m.t_ptr(x[k]) for k in COMPONENT_INPUTS[2]],
                                                 None, m.t_ptr(j), m.t_ptr(div), None, m.t_ptr(bad), m.current_stream_ptr(device)))
    return div, j, bad.bool()


def plume_model(device, compression=None):
    def run(inputs, n):                                   # pem_plume_f64_dev [+ pem_svd_compress_f64_dev] -> [n][div_angle, latents]
        import torch
        div, j, _ = plume_run(inputs, n, device)
        y = div.reshape(n, 1)
        return torch.cat([y, compression.compress(j)], dim=1) if compression is not None else y
    return run


def box_points(varied, fixed, priors, domains, num: int, seed: int):
    """`num` uniform points of a component's box in physical units, drawn and mapped as SparseGridSurrogate._fit_compression
    and SparseGridSurrogate.to_physical do"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1.0, 1.0, (len(varied), int(num)))
    full = {k: np.full(int(num), float(fixed[k])) for k in fixed}
    for d, k in enumerate(varied):
        u = 0.5 * (t[d] + 1.0)
        if k in domains:
            lo, hi = domains[k]
            full[k] = lo + (hi - lo) * u
        else:
            p = priors[k]
            v = p.a + (p.b - p.a) * u
            full[k] = 10.0 ** v if p.kind == sampling.LOGUNIFORM else v
    return full


def coupling_domain(y):
    """[min - 0.05 w, max + 0.05 w], w = max(max - min, 1e-3 max(|min|, |max|)): a constant output gets a narrow domain"""
    lo, hi = float(np.min(y)), float(np.max(y))
    w = max(hi - lo, 1e-3 * max(abs(lo), abs(hi)))
    return lo - 0.05 * w, hi + 0.05 * w


class ChainedSurrogate:
    """The three component surrogates, their coupling domains and the shared coordinate numbering of the chained launch:
    slots 0 .. n_ext - 1 are the varied external inputs in COUPLED_INPUTS order, then the V_cc slot, then the I_B0 slot."""

    def __init__(self, varied, fixed: dict | None = None, priors=None, field: bool = True, compression=None, seed: int = 0,
                 device=None, max_active: int = 5, max_level: int = 4, domains=None, u_ion=False, uion_grid=None):
        """field: the plume carries j_ion's SVD latents (`compression`: a fitted map of the system's j_ion; None: one is fitted
        on 500 plume-only evaluations over the plume's box, log10 norm, reconstruction_tol 0.01).  domains: (V_cc, I_B0)
        domains already known (a restored chain); None: estimated from the upstream true models.
        u_ion: the thruster carries the SVD latents of its ion velocity profile on `uion_grid` = (z0, z1, num_cells), default
        `likelihood.UION_GRID`: a fitted `SVDCompression` of it, or True: one is fitted on 500 thruster-only evaluations over the
        thruster's box (gen_data.py:73-76), norm linear(1e-3), reconstruction_tol 0.01 (yml:207-214)."""
        import torch
        from .compression import SVDCompression
        from .likelihood import UION_GRID
        grid = UION_GRID if uion_grid is None else uion_grid
        self.uion_grid = (float(grid[0]), float(grid[1]), int(grid[2]))
        self.u_compression = None
        self.priors = dict(sampling.PEM_V0_PRIORS if priors is None else priors)
        self.fixed = dict(fixed or {})
        self.varied = tuple(k for k in COUPLED_INPUTS if k in set(varied))
        if len(self.varied) != len(tuple(varied)) or any(k in self.fixed for k in self.varied):
            raise ValueError(f'varied: distinct inputs of {COUPLED_INPUTS} that are not fixed; got {tuple(varied)}')
        missing = [k for k in COUPLED_INPUTS if k not in self.varied and k not in self.fixed]
        if missing:
            raise ValueError(f'inputs neither varied nor fixed: {missing}')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.n_ext = len(self.varied)
        self.n_dim = self.n_ext + 2
        self.vcc_slot, self.ib0_slot = self.n_ext, self.n_ext + 1
        slot = {k: i for i, k in enumerate(self.varied)}
        slot.update(V_cc=self.vcc_slot, I_B0=self.ib0_slot)
        self.domains = [None, None] if domains is None else [tuple(map(float, d)) for d in domains]
        self.stages, self.slots = [], []
        models = (cathode_model(self.device), thruster_model(self.device))
        for c, inputs in enumerate(COMPONENT_INPUTS):
            up = COUPLING[c - 1] if c else None
            dom = {up: self.domains[c - 1]} if up else {}
            if up and self.domains[c - 1] is None:          # estimate_bounds: the upstream model over its own box
                prev = self.stages[-1]
                x = box_points(prev.varied, prev.fixed, prev.priors, prev.domains, NUM_BOUNDS, seed)
                y = prev.model(x, NUM_BOUNDS)[:, 0].cpu().numpy()
                prev.model_evals += NUM_BOUNDS
                self.domains[c - 1] = dom[up] = coupling_domain(y)
            cvar = tuple(k for k in inputs if k in self.varied or k == up)
            cfix = {k: self.fixed[k] for k in inputs if k in self.fixed}
            kw = dict(fixed=cfix, priors=self.priors, device=self.device, max_active=max_active, max_level=max_level, inputs=inputs,
                      domains=dom, n_coords=self.n_dim)
            if c == 1 and u_ion is not False and u_ion is not None:
                comp, pre = u_ion, 0
                if comp is True:                            # 500 thruster-only evaluations over the thruster's box
                    from .models.thruster import thruster_analytic
                    x = _dev(box_points(cvar, cfix, self.priors, dom, 500, 0), inputs, self.device)
                    u = thruster_analytic(x, num_cells=self.uion_grid[2], domain=self.uion_grid[:2])['u_ion']
                    comp = SVDCompression(norm='linear', scale=1e-3, reconstruction_tol=0.01).fit(u.reshape(500, -1))
                    pre = 500
                if comp.basis is None or comp.basis.shape[0] != self.uion_grid[2] or not 1 <= comp.rank <= 14:
                    raise ValueError(f'the u_ion map must be fitted on the {self.uion_grid[2]}-cell profile with 1 <= rank <= 14')
                self.u_compression = comp
                qoi = COMPONENT_OUTPUTS[c] + tuple(f'u_ion_latent{q}' for q in range(comp.rank))
                s = SparseGridSurrogate(cvar, qoi=qoi, model=thruster_model(self.device, comp, self.uion_grid), **kw)
                s.model_evals += pre
            elif c < 2:
                s = SparseGridSurrogate(cvar, qoi=COMPONENT_OUTPUTS[c], model=models[c], **kw)
            else:
                comp, pre = compression, 0
                if field and comp is None:                  # 500 plume-only evaluations over the plume's box (gen_data.py:73-76)
                    _, j, bad = plume_run(box_points(cvar, cfix, self.priors, dom, 500, 0), 500, self.device)
                    comp = SVDCompression(norm='log10', reconstruction_tol=0.01).fit(j[~bad])     # gen_data.py:277 drops invalid samples
                    pre = 500
                qoi = COMPONENT_OUTPUTS[c] + (('j_ion',) if field else ())
                s = SparseGridSurrogate(cvar, qoi=qoi, model=plume_model(self.device, comp if field else None), compression=comp, **kw)
                s.model_evals += pre
            self.stages.append(s)
            self.slots.append(np.array([slot[k] for k in cvar], dtype=np.int32))
        self.field = 'j_ion' if field else None
        self.compression = self.stages[2].compression
        self._tables = None

    # ---- bookkeeping -----------------------------------------------------------------------------------------------
    @property
    def model_evals(self):
        """per component: true-model evaluations so far"""
        return [s.model_evals for s in self.stages]

    def cost_weighted_evals(self):
        return float(sum(e * w for e, w in zip(self.model_evals, COST_SHARES)))

    def refine_step(self, num_refine: int = 1000, seed: int = 0):
        """One iteration of the cost-weighted greedy allocation: every component's candidates scored over `num_refine` points of
        its own box (one grid_values launch each), the (component, candidate) with the largest indicator / (nodes x share)
        activated.  Returns (component, beta, raw indicator, largest raw indicator) or None when no component has candidates."""
        import torch
        best = None
        top = 0.0
        for c, s in enumerate(self.stages):
            if not s.candidates:
                continue
            g = torch.Generator(device=self.device)
            g.manual_seed(seed * 3 + c)
            t = torch.rand((s.D, num_refine), dtype=torch.float64, device=self.device, generator=g) * 2 - 1
            cands, errs = s.candidate_indicators(t)
            for beta, e in zip(cands, errs):
                gain = float(e) / (s.values[beta].shape[0] * COST_SHARES[c])
                top = max(top, float(e))
                if best is None or gain > best[0]:
                    best = (gain, c, beta, float(e))
        if best is None:
            return None
        _, c, beta, e = best
        self.stages[c]._activate(beta)
        self._tables = None
        return c, beta, e, top

    # ---- the chained launch ----------------------------------------------------------------------------------------
    def stage_tables(self):
        """the three device tables with dims[] renumbered to shared coordinate slots: ([pem_surr_stage] * 3, keep-alive)"""
        import torch
        if self._tables is None:
            st, keep = (_lib.SurrStage * 3)(), []
            for k, (s, slots) in enumerate(zip(self.stages, self.slots)):
                idx, coef, vals, nb, na, lv = s._tables_for(None)
                h = idx.cpu().numpy().copy()
                for r in range(h.shape[0]):
                    h[r, 2:2 + h[r, 0]] = slots[h[r, 2:2 + h[r, 0]]]
                idx = torch.from_numpy(h).to(self.device)
                keep += [idx, coef, vals]
                st[k] = _lib.SurrStage(idx.data_ptr(), coef.data_ptr(), vals.data_ptr(), nb, s.n_out, na, lv)
            self._tables = (st, keep)
        return self._tables

    def predict(self, t, field: bool = True):
        """t: [n_ext][n] normalised external coordinates -> (out [5 + latents][n]: V_cc, I_B0, T, div_angle, T_c, latents...;
        field [n][91] or None), ONE pem_sparse_predict_chain_f64_dev launch.  A chain that carries u_ion appends its latents' rows
        (`pem_sparse_predict_chain_fields_f64_dev`); `predict_fields` gives the profile."""
        if self.u_compression is not None:
            return self._predict_uion(t, field, False)[:2]
        import torch
        st, _keep = self.stage_tables()
        t = t.to(device=self.device, dtype=torch.float64).contiguous()
        n = t.shape[1]
        p3 = self.stages[2]
        out = torch.empty((4 + p3.n_out, n), dtype=torch.float64, device=self.device)
        rebuild = bool(field and self.field)
        fld = torch.empty((n, FIELDS['j_ion']), dtype=torch.float64, device=self.device) if rebuild else None
        c = self.compression
        basis = c.basis.contiguous() if rebuild else None
        (vlo, vhi), (ilo, ihi) = self.domains
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None                                 # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_sparse_predict_chain_f64_dev(
                n, self.n_dim, self.vcc_slot, self.ib0_slot, st, vlo, vhi - vlo, ilo, ihi - ilo, p(t), max(t.stride(0), n), p(out),
                out.stride(0), 1 if rebuild else 0, c.rank if rebuild else 0, FIELDS['j_ion'], c.norm if rebuild else 0,
                c.scale if rebuild else 1.0, p(basis), p(fld), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out, fld

    def _predict_uion(self, t, field: bool, u_field: bool):
        """`predict` of a chain that carries u_ion: (out [4 + plume outputs + u_rank][n], j_ion [n][91] or None, u_ion [n][num_cells]
        or None), ONE pem_sparse_predict_chain_fields_f64_dev launch"""
        import torch
        st, _keep = self.stage_tables()
        t = t.to(device=self.device, dtype=torch.float64).contiguous()
        n = t.shape[1]
        c, cu = self.compression, self.u_compression
        out = torch.empty((4 + self.stages[2].n_out + cu.rank, n), dtype=torch.float64, device=self.device)
        rebuild = bool(field and self.field)
        fld = torch.empty((n, FIELDS['j_ion']), dtype=torch.float64, device=self.device) if rebuild else None
        ufld = torch.empty((n, self.uion_grid[2]), dtype=torch.float64, device=self.device) if u_field else None
        basis = c.basis.contiguous() if rebuild else None
        ubasis = cu.basis.contiguous()
        (vlo, vhi), (ilo, ihi) = self.domains
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None                                 # noqa: E731
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pem_sparse_predict_chain_fields_f64_dev(
                n, self.n_dim, self.vcc_slot, self.ib0_slot, st, vlo, vhi - vlo, ilo, ihi - ilo, p(t), max(t.stride(0), n), p(out),
                out.stride(0), 1 if rebuild else 0, c.rank if rebuild else 0, FIELDS['j_ion'], c.norm if rebuild else 0,
                c.scale if rebuild else 1.0, p(basis), p(fld), 2, cu.rank, self.uion_grid[2], cu.norm, cu.scale, p(ubasis), p(ufld),
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out, fld, ufld

    def uion_coords(self):
        """the (num_cells,) axial positions of the u_ion profile: the kernels' own grid doubles (pem_thruster_uion_f64_dev's z)"""
        from .models.thruster import thruster_analytic
        import torch
        one = {k: torch.ones(1, dtype=torch.float64, device=self.device) for k in COMPONENT_INPUTS[1]}
        return thruster_analytic(one, num_cells=self.uion_grid[2], domain=self.uion_grid[:2])['u_ion_coords']

    def run_system_loglik(self, t, likelihood, a_1=None, discharge=None, out=None, pred=None, qoi=None):
        """The chain and the multi-QoI log-likelihood of a `likelihood.SystemLikelihood` in ONE launch
        (`pem_chain_system_loglik_f64_dev`): the surrogate in the model's place, as the reference calibrates (mcmc.py:57-106).
        t: [n_ext][n] normalised external coordinates (unit column stride); sample i belongs to condition i mod n_cond.
        a_1, discharge: the (n,) anomalous-transport inputs and (I_d, sigma): the discharge-current term with I_d = I_B0 /
        (1 - 2 a_1) from the surrogate's I_B0 is added to every sample (both or neither).
        out: the (n,) per-sample sums (allocated when None; returned).  pred: a (ceil(n / n_cond), >= n_rec) tensor that receives
        the model value of every record.  qoi: a (4 + plume outputs, >= n) tensor that receives the rows of `predict`.
        The j_ion map (norm, scale, rank, basis) is this chain's compression; without one (`field=False`) j_ion records give NaN.
        A chain that carries u_ion serves the u_ion records too (`pem_chain_fields_loglik_f64_dev`; `qoi` then has its latents' rows
        as well); the likelihood's `uion_grid` must be the chain's.  Without it they give NaN."""
        import torch
        lk = likelihood
        if len(lk.sweep_radii) > 1:         # (the radius bits of its j_ion records must never reach pem_chain_*)
            raise ValueError(f'the likelihood holds j_ion at several sweep radii {lk.sweep_radii}: the plume surrogate is trained at '
                             f'one radius')
        st, _keep = self.stage_tables()

        def f64(x, what):
            if x.dtype != torch.float64 or x.device != self.device:
                raise ValueError(f'{what} must be a float64 tensor on {self.device}')
            return True
        f64(t, 't')
        if t.dim() != 2 or t.shape[0] != self.n_ext or (t.shape[0] and t.stride(1) != 1):
            raise ValueError(f't must be [{self.n_ext}][n] with unit column stride, got {tuple(t.shape)}')
        n = t.shape[1]
        if (a_1 is None) != (discharge is None):
            raise ValueError('the discharge term needs both a_1 and discharge = (I_d, sigma)')
        if a_1 is not None:
            f64(a_1, 'a_1')
            if a_1.shape != (n,) or not a_1.is_contiguous():
                raise ValueError(f'a_1 must be a contiguous ({n},) tensor')
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=self.device)
        f64(out, 'out')
        if out.shape != (n,) or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous ({n},) tensor')
        rows = -(-n // lk.n_cond)
        if pred is not None and (f64(pred, 'pred') and (pred.dim() != 2 or pred.stride(1) != 1 or pred.shape[0] < rows
                                                        or pred.shape[1] < lk.n_rec)):
            raise ValueError(f'pred must be a ({rows}, >= {lk.n_rec}) tensor with unit column stride')
        cu = self.u_compression
        if cu is not None and 'uion' in lk.qois and tuple(lk.uion_grid) != self.uion_grid:
            raise ValueError(f"the likelihood's u_ion grid {tuple(lk.uion_grid)} is not the chain's {self.uion_grid}: the latents rebuild "
                             f'the profile on the grid they were fitted on')
        n_plume = self.stages[2].n_out + (cu.rank if cu is not None else 0)
        if qoi is not None and (f64(qoi, 'qoi') and (qoi.dim() != 2 or qoi.stride(1) != 1 or qoi.shape[0] < 4 + n_plume
                                                     or qoi.shape[1] < n)):
            raise ValueError(f'qoi must be a ({4 + n_plume}, >= {n}) tensor with unit column stride')
        c = self.compression if self.field else None
        basis = c.basis.contiguous() if c is not None else None
        (vlo, vhi), (ilo, ihi) = self.domains
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None                                 # noqa: E731
        d = discharge if discharge is not None else (0.0, 1.0)
        args = (n, self.n_dim, self.vcc_slot, self.ib0_slot, st, vlo, vhi - vlo, ilo, ihi - ilo, p(t), max(t.stride(0), n) if self.n_ext else n,
                1, c.rank if c is not None else 0, FIELDS['j_ion'], c.norm if c is not None else 0, c.scale if c is not None else 1.0,
                p(basis), lk.n_cond, lk.n_rec, p(lk.rec), p(lk.span), p(a_1), float(d[0]), float(d[1]), p(out),
                p(qoi), qoi.stride(0) if qoi is not None else 0, p(pred), pred.stride(0) if pred is not None else 0)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            if cu is None:
                _lib.check(_lib.load().pem_chain_system_loglik_f64_dev(*args, stream))
            else:
                ubasis = cu.basis.contiguous()
                node_h = np.ascontiguousarray(lk.node_host, dtype=np.int32)          # what the entry point checks (host memory)
                _lib.check(_lib.load().pem_chain_fields_loglik_f64_dev(
                    *args, 2, cu.rank, self.uion_grid[2], cu.norm, cu.scale, p(ubasis), lk.n_node, p(lk.node),
                    node_h.ctypes.data_as(C.c_void_p), stream))
        return out

    def predict_fields(self, t):
        """t: [n_ext][n] -> {V_cc, I_B0, T, div_angle, T_c: (n,)[, j_ion: (n, 91), j_ion_latent: (n, rank)][, u_ion: (n, num_cells),
        u_ion_latent: (n, u_rank), u_ion_coords: (num_cells,)]}"""
        if self.u_compression is None:
            out, fld = self.predict(t)
        else:
            out, fld, ufld = self._predict_uion(t, True, True)
        res = {k: out[i] for i, k in enumerate(CHAIN_OUTPUTS)}
        n_plume = self.stages[2].n_out
        if self.field:
            res['j_ion'] = fld
            res['j_ion_latent'] = out[5:4 + n_plume].T
        if self.u_compression is not None:
            res['u_ion'] = ufld
            res['u_ion_latent'] = out[4 + n_plume:].T
            res['u_ion_coords'] = self.uion_coords()
        return res

    # ---- persistence ------------------------------------------------------------------------------------------------
    def state(self):
        return {'varied': self.varied, 'fixed': self.fixed, 'field': self.field, 'domains': self.domains,
                'compression': _compression_state(self.compression), 'u_ion': _compression_state(self.u_compression),
                'uion_grid': self.uion_grid,
                'stages': [{'index_set': s.index_set, 'candidates': s.candidates, 'values': s.values, 'model_evals': s.model_evals,
                            'max_active': s.max_active, 'max_level': s.max_level} for s in self.stages]}

    @classmethod
    def from_state(cls, st, priors=None):
        comp = _compression_from_state(st['compression'])
        ucomp = _compression_from_state(st.get('u_ion'), norm='linear')
        g = st['stages'][0]
        self = cls(st['varied'], st['fixed'], priors=priors, field=st['field'] is not None, compression=comp, domains=st['domains'],
                   max_active=g['max_active'], max_level=g['max_level'], u_ion=ucomp if ucomp is not None else False,
                   uion_grid=st.get('uion_grid'))
        for s, g in zip(self.stages, st['stages']):
            s.index_set, s.candidates, s.values, s.model_evals = g['index_set'], g['candidates'], g['values'], g['model_evals']
            s.rebuild_device_tables()
        self._tables = None
        return self
