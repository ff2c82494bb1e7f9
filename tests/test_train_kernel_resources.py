"""Code-object hygiene of the three kernels of training through the solve (no GPU): scratch, spill and LDS figures read from the
library's metadata notes with tools/kernel_resources.py, as tests/test_ensemble_kernel_resources.py does for the ensemble step.  None
of them uses scratch or spills a register; the only LDS is the norm kernel's workgroup fold, four fp64 words."""
import importlib
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

KERNELS = {"ionode::ionode_train_grad_norm_kernel(ionode::TrNormArgs)": 32,
           "ionode::ionode_train_apply_kernel(ionode::TrApplyArgs)": 0,
           "ionode::ionode_train_refresh_kernel(ionode::TrRefreshArgs)": 0}     # kernel: bytes of static LDS


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_train_kernels_use_no_scratch_and_spill_nothing():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    from kernel_resources import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources(ion.capi.LIB_PATH) if "ionode_train_" in r["kernel"]}
    assert sorted(rows) == sorted(KERNELS), sorted(rows)
    for name, lds in KERNELS.items():
        r = rows[name]
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["agpr"] == 0, r
        assert r["lds_static"] == lds, r
        assert r["vgpr"] <= 64, r          # 256-lane workgroups at full occupancy: nothing here holds state in registers
