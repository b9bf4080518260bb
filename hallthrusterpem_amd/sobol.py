"""Definition of the Sobol' study of scripts/pem_v0/sobol.py:46-118 (`compute_indices`) over a sweep of background pressures:
the nominal values of the 15 coupled inputs, the QoI groups and the inputs each varies, and the per-pressure prior tables.
`drivers.sobol_sweep` runs the study (csrc/pem_sobol_sweep.hip).

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
