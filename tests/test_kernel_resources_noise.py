"""Static resources of the scaled marginal (csrc/pem_likelihood.hip), checked where it is compiled (no GPU needed: hipcc
cross-compiles gfx950).  Both instances of loglik_marginal_scaled_kernel -- with and without the ess / chi accumulators: no
scratch, no spilled vector register (the group tables are indexed by unrolled constants only, so nothing lands in private memory),
the row's weights and the wave partials in a few hundred bytes of static LDS, and registers within what four waves per SIMD
leave: the launch is one 256-thread workgroup per chain and latency-bound, several of them share a CU."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_likelihood.hip'
VGPRS_PER_LANE = 512
KERNELS = ['loglik_marginal_scaled_kernel<false>', 'loglik_marginal_scaled_kernel<true>']


def _rows():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(SRC), '--grep', 'loglik_marginal'],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)), lds=int(m.group(8)))
    return rows


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_the_scaled_marginal_has_no_scratch_no_vector_spill_and_a_few_lds_words():
    rows = _rows()
    assert sorted(k for k in rows if 'scaled' in k) == KERNELS, rows
    for name in KERNELS:
        r = rows[name]
        assert r['scratch'] == 0 and r['vspill'] == 0, (name, r)
        assert r['lds'] <= 1024, (name, r)
        assert r['vgpr'] <= VGPRS_PER_LANE // 4, (name, r)
    # the unscaled kernel stays as it was: the scale-1 contract compares against it
    assert rows['loglik_marginal_kernel']['scratch'] == 0 and rows['loglik_marginal_kernel']['lds'] == 64, rows
