"""Static resources of the conditional information launch (csrc/pem_information_theta.hip), checked where it is compiled (no GPU
needed: hipcc cross-compiles gfx950).  Its one kernel: no scratch, no spilled vector register, static LDS within the 160 KiB of a
CU, and registers and LDS within what the declared `amdgpu_waves_per_eu` and workgroup size allow -- 512 vector registers per SIMD
lane shared by the waves, and a workgroup's waves spread over the 4 SIMDs of a CU."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_information_theta.hip'
LDS_PER_CU = 163_840
VGPRS_PER_LANE = 512


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
    """kernel -> (threads of its workgroup, declared waves per SIMD): the kernel declares __launch_bounds__ and amdgpu_waves_per_eu
    with named constants, the same one for both bounds of the occupancy"""
    text = SRC.read_text()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (\w+) = (\d+);', text)}
    found = re.findall(r'__launch_bounds__\((\w+)\)\s*__attribute__\(\(amdgpu_waves_per_eu\((\w+), (\w+)\)\)\)\s*void\s+(\w+)\s*\(', text)
    assert len(found) == text.count('__global__') == 1, found
    assert all(lo == hi and not lo.isdigit() and not threads.isdigit() for threads, lo, hi, _ in found), found
    return {name: (const[threads], const[lo]) for threads, lo, _, name in found}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_the_conditional_kernel_has_no_scratch_no_vector_spill_and_fits_its_declared_occupancy():
    rows, declared = _rows(), _declared()
    assert sorted(rows) == ['conditional_lse_kernel'] == sorted(declared), rows
    for name, r in rows.items():
        threads, waves = declared[name]
        assert r['scratch'] == 0 and r['vspill'] == 0, (name, r)
        assert r['lds'] <= LDS_PER_CU, (name, r)
        assert r['vgpr'] <= VGPRS_PER_LANE // waves, (name, r, waves)
        # a workgroup is one wave: it is on one SIMD, and the declaration cannot promise less than that one wave
        assert threads == 64 and waves >= 1, (name, threads, waves)
        # the workgroups the LDS admits on a CU carry at least the declared waves per SIMD
        assert r['lds'] > 0 and (LDS_PER_CU // r['lds']) * (threads // 64) >= 4 * waves, (name, r, waves)
