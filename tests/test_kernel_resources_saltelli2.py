"""Static resources of the second-order Saltelli launch (csrc/pem_saltelli2.hip), checked where it is compiled (no GPU needed: hipcc
cross-compiles gfx950).  Every kernel of the file: no scratch, no spilled vector register, static LDS within the 160 KiB of a CU,
and registers within what its declared `amdgpu_waves_per_eu` allows -- 512 vector registers per SIMD lane shared by the waves."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / 'hallthrusterpem_amd' / 'csrc' / 'pem_saltelli2.hip'
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


def _declared_waves():
    """kernel<Model> -> the waves per SIMD its amdgpu_waves_per_eu attribute declares: every kernel of the file declares
    `S2_WAVES<Model>` for both bounds, and the file defines that as 2 for the model whose real type has four bytes, 1 otherwise"""
    text = SRC.read_text()
    assert re.search(r'constexpr int S2_WAVES = sizeof\(typename Model::real\) == 4 \? 2 : 1;', text)
    found = re.findall(r'amdgpu_waves_per_eu\(S2_WAVES<Model>, S2_WAVES<Model>\)\)\)\s*void\s+(\w+)\s*\(', text)
    assert len(found) == text.count('__global__') == 2, found
    return {f'{name}<{model}>': waves for name in found for model, waves in (('Model32', 2), ('Model64', 1))}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_every_second_order_kernel_has_no_scratch_no_vector_spill_and_fits_its_declared_occupancy():
    rows, waves = _rows(), _declared_waves()
    assert sorted(rows) == ['saltelli2_kernel<Model32>', 'saltelli2_kernel<Model64>', 'saltelli2_qmc_kernel<Model32>',
                            'saltelli2_qmc_kernel<Model64>'], rows
    for name, r in rows.items():
        w = waves[name]
        assert r['scratch'] == 0 and r['vspill'] == 0, (name, r)
        assert r['lds'] <= LDS_PER_CU, (name, r)
        assert r['vgpr'] <= VGPRS_PER_LANE // w, (name, r, w)
        # the workgroups the LDS admits on a CU carry at least the declared waves per SIMD (4 waves a workgroup, 4 SIMDs a CU)
        assert LDS_PER_CU // r['lds'] >= w, (name, r, w)
