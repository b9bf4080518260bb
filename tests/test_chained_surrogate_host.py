"""The component chain's C ABI and its numpy restatement, without a GPU: pem_sparse_predict_chain_f64_dev is declared and bound,
refuses every malformed call before it looks for a device, and tests/chain_np.py composes three stages exactly."""
import ctypes as C
import itertools
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
NAME = 'pem_sparse_predict_chain_f64_dev'


def test_symbol_is_declared_and_bound():
    from hallthrusterpem_amd import _lib
    header = (ROOT / 'include' / 'pem_hip.h').read_text()
    assert re.search(r'\bint\s+%s\s*\(' % NAME, header) and 'typedef struct pem_surr_stage' in header
    assert NAME in _lib.SIGNATURES
    assert hasattr(_lib.load(), NAME)
    assert C.sizeof(_lib.SurrStage) == 3 * 8 + 4 * 4


def _call(stages=True, n=1000, n_dim=4, vcc_slot=2, ib0_slot=3, vcc=(0.0, 1.0), ib0=(0.0, 1.0), t=True, ld=1000, out=True,
          ld_out=1000, field=False, lat0=1, rank=1, dof=91, norm=1, basis=True, outs=(1, 2, 3), active=(5, 5, 5), level=(4, 4, 4),
          null_table=None):
    from hallthrusterpem_amd import _lib
    fake = C.c_void_p(4096)                     # never dereferenced: every check below runs on the host
    arr = (_lib.SurrStage * 3)()
    for k in range(3):
        ptrs = [fake.value] * 3
        if null_table == k:
            ptrs[k % 3] = None
        arr[k] = _lib.SurrStage(ptrs[0], ptrs[1], ptrs[2], 3, outs[k], active[k], level[k])
    return _lib.load().pem_sparse_predict_chain_f64_dev(
        n, n_dim, vcc_slot, ib0_slot, arr if stages else None, vcc[0], vcc[1], ib0[0], ib0[1], fake if t else None, ld,
        fake if out else None, ld_out, lat0, rank, dof, norm, 1.0, fake if basis else None, fake if field else None, None)


@pytest.mark.parametrize('bad', [
    dict(stages=False), dict(null_table=0), dict(null_table=1), dict(null_table=2),
    dict(outs=(0, 2, 3)), dict(outs=(2, 2, 3)), dict(outs=(1, 1, 3)), dict(outs=(1, 3, 3)), dict(outs=(1, 2, 0)), dict(outs=(1, 2, 17)),
    dict(active=(6, 5, 5)), dict(level=(4, 5, 4)), dict(active=(5, 5, -1)),
    dict(vcc_slot=4), dict(ib0_slot=-1), dict(vcc_slot=3), dict(n_dim=1), dict(n_dim=33),
    dict(vcc=(0.0, 0.0)), dict(vcc=(0.0, -1.0)), dict(ib0=(0.0, float('nan'))), dict(ib0=(0.0, float('inf'))), dict(vcc=(float('nan'), 1.0)),
    dict(field=True, rank=0), dict(field=True, rank=17), dict(field=True, lat0=1, rank=3), dict(field=True, lat0=-1),
    dict(field=True, dof=0), dict(field=True, basis=False), dict(field=True, norm=7),
    dict(t=False), dict(out=False), dict(ld=999), dict(ld_out=999),
    dict(n_dim=13),                              # 4 outer dimensions of 17 nodes and 13 coordinates: 162 KB of LDS
])
def test_malformed_calls_are_refused_without_a_device(bad):
    from hallthrusterpem_amd import _lib
    assert _call(**bad) == _lib.PEM_ERR_INVALID_ARG, bad
    assert b'pem_sparse_predict_chain' in _lib.load().pem_last_error()


def test_a_well_formed_call_needs_the_device():
    from hallthrusterpem_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip('a HIP device is present')
    assert _call() == _lib.PEM_ERR_NO_DEVICE
    assert _call(n_dim=12, field=True, lat0=1, rank=2) == _lib.PEM_ERR_NO_DEVICE          # 160 KB exactly
    assert _call(n_dim=2, vcc_slot=0, ib0_slot=1, t=False, ld=0) == _lib.PEM_ERR_NO_DEVICE                            # no external coordinate
    assert _call(n=0, t=False, out=False) == _lib.PEM_OK


# ---- chain_np on a hand-built chain whose stages interpolate low-degree polynomials exactly -----------------------------------
def _tensor_stage(n_dim, levels_at, fns):
    """one grid of the given {slot: level} whose node values are fns(t) (each of degree < nodes per slot): the interpolant is fns"""
    sys.path.insert(0, str(ROOT))
    from oracle import surrogate_np as snp
    beta = tuple(levels_at.get(d, 0) for d in range(n_dim))
    pts = np.array(list(itertools.product(*[snp.nodes(l) for l in beta]))).T
    vals = np.stack([f(pts) for f in fns], axis=1)
    return [beta], {beta: 1.0}, {beta: vals}


def test_chain_np_composes_exactly():
    import chain_np
    n_dim, vs, ib = 4, 2, 3                                   # slots 0, 1 external, then V_cc, I_B0
    vcc_f = lambda t: 20.0 + 5.0 * t[0] + 2.0 * t[0] * t[1] + 3.0 * t[1] ** 2          # noqa: E731
    ib0_f = lambda t: 3.0 + 0.1 * t[2] + 0.05 * t[0] * t[2]                               # noqa: E731
    thr_f = lambda t: 0.08 + 0.01 * t[2] ** 2                                             # noqa: E731
    div_f = lambda t: 0.3 + 0.05 * t[3] - 0.02 * t[1] * t[3] ** 3                         # noqa: E731
    lat_f = lambda t: -1.5 + 0.25 * t[3] ** 2 * t[1]                                      # noqa: E731
    stages = [_tensor_stage(n_dim, {0: 1, 1: 2}, [vcc_f]), _tensor_stage(n_dim, {0: 1, 2: 2}, [ib0_f, thr_f]),
              _tensor_stage(n_dim, {1: 1, 3: 2}, [div_f, lat_f])]
    vmap, imap = (10.0, 25.0), (2.5, 1.0)
    rng = np.random.default_rng(5)
    te = rng.uniform(-1, 1, (2, 777))
    got = chain_np.compose(stages, te, vs, ib, vmap, imap)
    t = np.zeros((n_dim, te.shape[1]))
    t[:2] = te
    v = vcc_f(t)
    t[2] = 2.0 * (v - vmap[0]) / vmap[1] - 1.0
    i, thr = ib0_f(t), thr_f(t)
    t[3] = 2.0 * (i - imap[0]) / imap[1] - 1.0
    d, lat = div_f(t), lat_f(t)
    want = np.stack([v, i, thr, d, thr * np.cos(d), lat])
    assert got.shape == want.shape
    assert np.max(np.abs(got - want) / np.abs(want).max(axis=1, keepdims=True)) <= 1e-13
    ld = chain_np.compose_ld([(b, [c[b[0]]], [y[b[0]]]) for b, c, y in stages], te, vs, ib, vmap, imap)
    assert np.max(np.abs(ld.astype(np.float64) - want) / np.abs(want).max(axis=1, keepdims=True)) <= 1e-13


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc is not available')
def test_chain_kernels_neither_spill_vgprs_nor_use_scratch():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_surrogate.hip'),
                          '--grep', 'sparse_chain_kernel'], capture_output=True, text=True, check=True).stdout
    rows = [line for line in out.splitlines() if line.startswith('sparse_chain_kernel')]
    assert len(rows) == 6, out                                  # plume widths 1, 2, 3, 4 exact; 8, 16 guarded
    for line in rows:
        g = lambda k: int(re.search(k + r'\s+(\d+)', line).group(1))              # noqa: E731
        assert g('v-spill') == 0 and g('scratch') == 0, line
        print(line[:40], 'SGPR spills:', g('s-spill'))          # reported, not gated
