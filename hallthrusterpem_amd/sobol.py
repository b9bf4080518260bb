"""Definition of the Sobol' study of scripts/pem_v0/sobol.py:46-118 (`compute_indices`) over a sweep of background pressures:
the nominal values of the 15 coupled inputs, the QoI groups and the inputs each varies, and the per-pressure prior tables.
`drivers.sobol_sweep` runs the study (csrc/pem_sobol_sweep.hip), around the model or, for the Cathode and Thruster groups, around
a trained `chain.ChainedSurrogate` (`surrogate_sweep_map`, csrc/pem_surrogate_sobol.hip) as the reference's model() does
(sobol.py:70-98).

Per QoI the reference varies only the exogenous inputs of the component that produces it (IDX_MAP, sobol.py:24-29); every
other input sits at its nominal value (sobol.py:73-80) and `V_a` (with `r_m`) is held constant (CONSTANTS).  The groups:

  Cathode   V_cc       the cathode stage                              P_b T_e V_vac Pstar P_T
  Thruster  T, uion    cathode -> the thruster test double            P_b mdot_a T_e a_1
  Plume     jion       the plume alone at I_B0 = 4 A, r = 1 m          P_b c0..c5 sigma_cex

The Thruster set is the YAML Thruster's exogenous inputs that exist in the 15-input model; `T_e` is listed under both Cathode
and Thruster.  `u_n`, `l_t`, `a_2`, `dz`, `z0` and `p0` belong to HallThruster.jl and are absent from the test double.

ASSUMPTION (amisc is absent, its samplers are unpinned): `Relative(x)` is read as uniform on nominal * (1 +- x / 100) in
linear units, intersected with the YAML domain.  `P_b` is Relative(20) around each pressure of the sweep (at 1e-4 Torr the
upper edge is clipped to the domain), `mdot_a` Relative(3) around 5e-6 kg/s; the calibration inputs keep their priors
(`sampling.PEM_V0_PRIORS`).
"""
import numpy as np

from . import sampling
from .models.coupled import COUPLED_INPUTS

# pem_v0_SPT-100.yml `nominal:` of each coupled input (tests/golden/pem_v0_variables.json pins them)
PEM_V0_NOMINAL = {
    'P_b': 1e-05, 'V_a': 300.0, 'T_e': 1.32721, 'V_vac': 31.61135, 'Pstar': 3.463406e-05, 'P_T': 1.019193e-05,
    'mdot_a': 5e-06, 'a_1': 0.00680237,
    'c0': 0.92434, 'c1': 0.81486, 'c2': 14.00547, 'c3': 0.44667, 'c4': 1e20, 'c5': 1e16, 'sigma_cex': 5.5e-19,
}
assert tuple(PEM_V0_NOMINAL) == COUPLED_INPUTS

DOMAINS = {'P_b': (1e-8, 1e-4), 'mdot_a': (2e-6, 7e-6)}          # yml:9-17, 113-121
RELATIVE = {'P_b': 20.0, 'mdot_a': 3.0}                           # percent, yml `distribution: Relative(x)`
CONSTANTS = ('V_a',)                                              # sobol.py:21 (r_m is the plume's fixed sweep radius)

GROUPS = ('Cathode', 'Thruster', 'Plume')                         # PEM_SWEEP_CATHODE, _THRUSTER, _PLUME: the kernel's order
GROUP_QOIS = {'Cathode': ('V_cc',), 'Thruster': ('T', 'uion'), 'Plume': ('jion',)}
GROUP_INPUTS = {'Cathode': ('P_b', 'T_e', 'V_vac', 'Pstar', 'P_T'),
                'Thruster': ('P_b', 'mdot_a', 'T_e', 'a_1'),
                'Plume': ('P_b', 'c0', 'c1', 'c2', 'c3', 'c4', 'c5', 'sigma_cex')}
QOIS = ('V_cc', 'T', 'uion', 'jion')
QOI_GROUP = {q: g for g, qs in GROUP_QOIS.items() for q in qs}
DEFAULT_PRESSURES = 10 ** np.linspace(-6, -4, 5)                  # sobol.py:99-100, Torr
PLUME_I_B0, PLUME_RADIUS = 4.0, 1.0                               # sobol.py:56-57, 82-85
L_CH = 0.025                                                      # sobol.py:23, m


def relative(nominal: float, percent: float, domain) -> sampling.Prior:
    """Relative(percent) around `nominal`: uniform on nominal * (1 -+ percent / 100), intersected with `domain` (an assumption,
    see the module docstring)."""
    lo, hi = nominal * (1 - percent / 100), nominal * (1 + percent / 100)
    return sampling.Prior(sampling.UNIFORM, max(lo, domain[0]), min(hi, domain[1]), f'Relative({percent:g}) around {nominal:g}')


def pin(value: float) -> sampling.Prior:
    """An input held at `value`: U(value, value), as `sobol_indices(fixed=...)` pins inputs."""
    return sampling.Prior(sampling.UNIFORM, float(value), float(value), 'pinned')


def sweep_priors(pressure: float, group: str) -> dict:
    """The 15 priors of `group` at background pressure `pressure` [Torr]: its varied inputs drawn (P_b and mdot_a Relative,
    the calibration inputs from their priors), every other input pinned at PEM_V0_NOMINAL."""
    if group not in GROUP_INPUTS:
        raise ValueError(f'unknown group {group!r}: one of {GROUPS}')
    varied = GROUP_INPUTS[group]
    out = {}
    for k in COUPLED_INPUTS:
        if k not in varied:
            out[k] = pin(PEM_V0_NOMINAL[k])
        elif k == 'P_b':
            out[k] = relative(float(pressure), RELATIVE[k], DOMAINS[k])
        elif k in RELATIVE:
            out[k] = relative(PEM_V0_NOMINAL[k], RELATIVE[k], DOMAINS[k])
        else:
            out[k] = sampling.PEM_V0_PRIORS[k]
    return out


def prior_tables(pressures, group: str):
    """(kind int32 [P][15], a float64 [P][15], b float64 [P][15]): the tables pem_sobol_sweep_f64_dev reads."""
    rows = [sweep_priors(p, group) for p in pressures]
    kind = np.array([[r[k].kind for k in COUPLED_INPUTS] for r in rows], dtype=np.int32)
    a = np.array([[r[k].a for k in COUPLED_INPUTS] for r in rows], dtype=np.float64)
    b = np.array([[r[k].b for k in COUPLED_INPUTS] for r in rows], dtype=np.float64)
    return kind, a, b


def uion_node(l_ch: float, uion_grid):
    """(index, z) of the node of the u_ion grid z_c = z0 + (z1 - z0) (c / (num_cells - 1)) nearest to `l_ch`
    (sobol.py:94: argmin |z - L_ch|)."""
    z0, z1, ncells = float(uion_grid[0]), float(uion_grid[1]), int(uion_grid[2])
    if not (ncells >= 2 and z1 > z0):
        raise ValueError(f'uion_grid = (z0, z1, num_cells) needs z1 > z0 and num_cells >= 2, got {tuple(uion_grid)}')
    if not (np.isfinite(l_ch) and z0 <= l_ch <= z1):
        raise ValueError(f'l_ch = {l_ch} lies outside the u_ion grid [{z0}, {z1}]')
    z = z0 + (z1 - z0) * (np.arange(ncells, dtype=np.float64) / np.float64(ncells - 1))
    c = int(np.argmin(np.abs(z - l_ch)))
    return c, float(z[c])


def row_stream(group: int, n_p: int, p: int, attempt: int, row: int) -> int:
    """Stream of attempt `attempt` of row `row` (0: A, 1: B) of group `group` at pressure index `p` (include/pem_hip.h)."""
    return 2 * len(GROUPS) * n_p * attempt + 2 * (group * n_p + p) + row


# ---- the study through a chained surrogate (sobol.py:70-98: V_cc, T and u_ion come from SURR.predict) ---------------------------
SURROGATE_GROUPS = ('Cathode', 'Thruster')                        # the Plume group stays on the model (sobol.py:82-90)
# what each group's stages read: the cathode component's inputs, and for the Thruster group the thruster component's as well
_CATHODE_READS = ('P_b', 'V_a', 'T_e', 'V_vac', 'Pstar', 'P_T')
GROUP_READS = {'Cathode': _CATHODE_READS, 'Thruster': _CATHODE_READS + ('mdot_a', 'a_1')}


class SweepSlotMap:
    """How the rows of the study's design become the external coordinates of a chained surrogate: slot k reads input row
    `rows[k]`, u = log10(x) where `is_log[k]`, t = 2.0 * (u - a[k]) / w[k] - 1.0 with w = b - a formed here in float64.  The
    arrays are the slot table of `pem_chain_sobol_sweep_f64_dev`; `coords` is the numpy form of the map."""

    def __init__(self, rows, is_log, a, w):
        self.rows = np.ascontiguousarray(rows, dtype=np.int32)
        self.is_log = np.ascontiguousarray(is_log, dtype=np.int32)
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)

    def coords(self, x):
        """x: (15, n) physical inputs -> (n_ext, n) coordinates, left to right as the kernel forms them"""
        x = np.asarray(x, dtype=np.float64)
        t = np.empty((len(self.rows), x.shape[1]))
        for d, r in enumerate(self.rows):
            u = np.log10(x[r]) if self.is_log[d] else x[r]
            t[d] = 2.0 * (u - self.a[d]) / self.w[d] - 1.0
        return t


def _box_coordinate(prior: sampling.Prior, value: float) -> float:
    """`value` in the units a surrogate's box [prior.a, prior.b] is stated in (log10 for a log-uniform input)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.log10(value)) if prior.kind == sampling.LOGUNIFORM else float(value)


def surrogate_sweep_map(chain_varied, chain_fixed, chain_priors, pressures, group: str, has_uion: bool = False, qois=()):
    """The slot table of the study's `group` at `pressures` evaluated through a chained surrogate (`chain.ChainedSurrogate`: its
    `varied`, `fixed`, `priors` and whether it carries the u_ion latents).  Runs without a device.  ValueError, naming the input,
    for what the surrogate cannot serve: a varied input of the group it does not vary, an input the group's stages read that it
    fixes away from `PEM_V0_NOMINAL`, a pin or a sweep range outside its box, a normal prior, `uion` without latents.  Inputs
    that only the plume stage reads are not examined (the launch never runs that stage)."""
    if group not in SURROGATE_GROUPS:
        raise ValueError(f'group {group!r}: a chained surrogate serves the groups {SURROGATE_GROUPS}; the Plume group stays on the model')
    varied, fixed = tuple(k for k in COUPLED_INPUTS if k in set(chain_varied)), dict(chain_fixed)
    if 'uion' in qois and not has_uion:
        raise ValueError("'uion' is asked of a chain without u_ion latents (the thruster stage predicts I_B0 and T only): build it "
                         'with u_ion=True')
    tol = 8 * np.finfo(np.float64).eps
    inside = lambda u, p: p.a - tol * abs(p.a) <= u <= p.b + tol * abs(p.b)                      # noqa: E731
    sweeps = [sweep_priors(p, group) for p in np.atleast_1d(np.asarray(pressures, dtype=np.float64))]
    for k in GROUP_READS[group]:
        is_var = k in GROUP_INPUTS[group]
        if k in fixed:
            if is_var:
                raise ValueError(f"'{k}' is varied by the {group} group and the surrogate holds it fixed at {fixed[k]}")
            if float(fixed[k]) != PEM_V0_NOMINAL[k]:
                raise ValueError(f"the surrogate holds '{k}' fixed at {fixed[k]}; the study pins it at its nominal value {PEM_V0_NOMINAL[k]}")
            continue
        if k not in varied:
            raise ValueError(f"'{k}' is read by the {group} group and the surrogate neither varies nor fixes it (its varied inputs "
                             f'are {varied})')
        p = chain_priors[k]
        if p.kind == sampling.NORMAL:
            raise ValueError(f"'{k}': a surrogate's box is uniform or log-uniform, its prior is normal")
        box = (10.0 ** p.a, 10.0 ** p.b) if p.kind == sampling.LOGUNIFORM else (p.a, p.b)
        if not is_var:
            if not inside(_box_coordinate(p, PEM_V0_NOMINAL[k]), p):
                raise ValueError(f"'{k}' is pinned at {PEM_V0_NOMINAL[k]}, outside the surrogate's box [{box[0]}, {box[1]}]")
            continue
        for pres, row in zip(np.atleast_1d(pressures), sweeps):
            q = row[k]
            if q.kind == p.kind:
                lo, hi = q.a, q.b
            else:
                ends = (10.0 ** q.a, 10.0 ** q.b) if q.kind == sampling.LOGUNIFORM else (q.a, q.b)
                lo, hi = (_box_coordinate(p, v) for v in ends)
            if not (inside(lo, p) and inside(hi, p)):
                ends = (10.0 ** q.a, 10.0 ** q.b) if q.kind == sampling.LOGUNIFORM else (q.a, q.b)
                raise ValueError(f"'{k}' is swept over [{ends[0]}, {ends[1]}] at {float(pres):g} Torr, outside the surrogate's box "
                                 f'[{box[0]}, {box[1]}]')
    rows, is_log, a, w = [], [], [], []
    for k in varied:                                  # the chain's external slots: its varied inputs in COUPLED_INPUTS order
        p = chain_priors[k]
        rows.append(COUPLED_INPUTS.index(k))
        if p.kind != sampling.NORMAL:
            is_log.append(p.kind == sampling.LOGUNIFORM)
            a.append(p.a)
            w.append(np.float64(p.b) - np.float64(p.a))
        else:                                         # (a plume-only input, not examined: never read by the launch's stages)
            is_log.append(False)
            a.append(0.0)
            w.append(1.0)
    return SweepSlotMap(rows, is_log, a, w)
