"""Code-object hygiene of the adaptive-Metropolis step kernels (no GPU): register, scratch and LDS figures read from the library's
metadata notes with tools/kernel_resources.py, as tests/test_lm_kernel_resources.py does for the Levenberg-Marquardt step.  One lane
per chain keeps the packed lower triangle of the proposal's factor in registers -- 91 words at 13 coordinates -- and nothing in
scratch or LDS; the register figures of the build that ships are pinned (a compiler that changes them should be looked at)."""
import importlib
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

# n: registers a lane holds (architectural and accumulation registers together), of the shipped build
VGPR = {1: 42, 2: 56, 3: 67, 4: 82, 5: 103, 6: 108, 7: 128, 8: 164, 9: 170, 10: 235, 11: 336, 12: 272, 13: 296}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_step_kernels_use_no_scratch_and_no_lds_and_their_registers_are_pinned():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    from kernel_resources import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources(ion.capi.LIB_PATH) if "ionode_mcmc_step_kernel<" in r["kernel"]}
    assert sorted(rows) == sorted(f"void ionode::ionode_mcmc_step_kernel<{n}>(ionode::McArgs)" for n in range(1, ion.capi.MCMC_MAX_DIM + 1)), sorted(rows)
    got = {}
    for n in range(1, 14):
        r = rows[f"void ionode::ionode_mcmc_step_kernel<{n}>(ionode::McArgs)"]
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["lds_static"] == 0 and r["vgpr"] <= 512, r
        got[n] = r["vgpr"]
    assert got == VGPR, got
    assert got[5] <= 128     # p1 .. p4 and sigma, the reference's case: four wavefronts per SIMD
