"""Static resources of the Jacobian launches (csrc/pem_jacobian.hip), checked where they are compiled (no GPU needed: hipcc
cross-compiles gfx950).  Every kernel of the file: no scratch, no spilled vector register, static LDS within the 160 KiB of a CU,
registers within what its declared `amdgpu_waves_per_eu` allows -- 512 vector registers per SIMD lane shared by the waves -- and LDS
that admits the workgroups of four waves that put that many waves on each of the four SIMDs."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_jacobian.hip'
LDS_PER_CU = 163_840
VGPRS_PER_LANE = 512
KERNELS = ['coupled_jacobian_kernel', 'gradient_sums_kernel<false>', 'gradient_sums_kernel<true>']


def _rows():
    out = subprocess.run([sys.executable, str(ROOT / 'tools' / 'kernel_stats.py'), str(SRC)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r'(\S+)\s+vgpr\s+(\d+) sgpr\s+(\d+) s-spill\s+(\d+) v-spill\s+(\d+) scratch\s+(\d+) kernarg\s+(\d+) lds\s+(\d+)', line)
        if m:
            rows[m.group(1)] = dict(vgpr=int(m.group(2)), vspill=int(m.group(5)), scratch=int(m.group(6)), lds=int(m.group(8)))
    return rows


def _declared():
    """(waves per SIMD every kernel of the file declares, lanes of its workgroup)"""
    text = SRC.read_text()
    found = re.findall(r'__launch_bounds__\(WG\) __attribute__\(\(amdgpu_waves_per_eu\((\d+), (\d+)\)\)\)\s*void\s+(\w+)\s*\(', text)
    assert len(found) == text.count('__global__') == 2, found
    assert all(lo == hi for lo, hi, _ in found) and len({lo for lo, _, _ in found}) == 1, found
    wg = int(re.search(r'constexpr int WG = (\d+);', text).group(1))
    return int(found[0][0]), wg


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_every_jacobian_kernel_has_no_scratch_no_vector_spill_and_fits_its_declared_occupancy():
    rows, (waves, wg) = _rows(), _declared()
    assert sorted(rows) == KERNELS, rows
    assert wg == 256                                                   # four waves a workgroup: one per SIMD
    for name, r in rows.items():
        assert r['scratch'] == 0 and r['vspill'] == 0, (name, r)
        assert r['lds'] <= LDS_PER_CU, (name, r)
        assert r['vgpr'] <= VGPRS_PER_LANE // waves, (name, r, waves)
        assert LDS_PER_CU // r['lds'] >= waves, (name, r, waves)
