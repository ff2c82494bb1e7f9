"""Code-object hygiene of the Levenberg-Marquardt step kernels (no GPU): register and scratch figures read from the library's
metadata notes with tools/kernel_resources.py, as tests/test_kernel_resources.py does for the other kernels.  One lane per
candidate keeps the factor's lower triangle in registers: at 12 free parameters that is most of the file, and none of it may spill."""
import importlib
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_step_kernels_use_no_scratch_and_no_lds():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    from kernel_resources import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources(ion.capi.LIB_PATH) if "ionode_lm_step_kernel<" in r["kernel"]}
    assert sorted(rows) == sorted(f"void ionode::ionode_lm_step_kernel<{nf}>(ionode::LmArgs)" for nf in range(1, 13)), sorted(rows)
    for name, r in rows.items():
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["lds_static"] == 0 and r["vgpr"] <= 512, r
    four = rows["void ionode::ionode_lm_step_kernel<4>(ionode::LmArgs)"]
    assert four["vgpr"] <= 128, four     # the reference's four free parameters: four wavefronts per SIMD
