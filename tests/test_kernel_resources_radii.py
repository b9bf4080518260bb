"""Static resources of the fused multi-QoI likelihood at several sweep radii (`plume_r1_kernel` JMODE 8: the per-sample sums,
JMODE 9: the record predictions), checked where they are compiled (no GPU needed: hipcc cross-compiles gfx950).  They keep the
shape of the one-radius modes 6 and 7 -- two waves per SIMD, so at most 256 vector registers, no spilled vector register and no
scratch -- and the pairs {base(r), j_cex(r)} they add live in LDS, not in registers held across the rounds."""
import shutil
from pathlib import Path

import pytest

from test_kernel_resources import kernel_rows


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason='hipcc not available')
def test_the_several_radii_modes_use_no_scratch_and_spill_no_vector_register():
    rows = kernel_rows('pem_kernels.hip')
    for mode in (8, 9):
        k = rows.get(f'plume_r1_kernel<4, true, {mode}, false, 0, false>')
        assert k is not None, sorted(rows)
        assert k['vspill'] == 0 and k['scratch'] == 0 and k['vgpr'] <= 256, (mode, k)
