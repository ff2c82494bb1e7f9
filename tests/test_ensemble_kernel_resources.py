"""Code-object hygiene of the ensemble step kernels (no GPU): register, scratch and LDS figures read from the library's metadata notes
with tools/kernel_resources.py, as tests/test_mcmc_kernel_resources.py does for the adaptive-Metropolis step.  A lane holds one
walker's u, ut and xt with constant indices -- nothing in scratch, no spilled vector register -- and the workgroup's only LDS is the
one word "a start is bad"; the register figures of the build that ships are pinned (a compiler that changes them should be looked at)."""
import importlib
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

# n: registers a lane holds (architectural and accumulation registers together), of the shipped build
VGPR = {1: 49, 2: 56, 3: 70, 4: 76, 5: 86, 6: 93, 7: 103, 8: 109, 9: 120, 10: 126, 11: 136, 12: 142, 13: 152}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_step_kernels_use_no_scratch_and_spill_nothing_and_their_registers_are_pinned():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    from kernel_resources import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources(ion.capi.LIB_PATH) if "ionode_ensemble_step_kernel<" in r["kernel"]}
    assert sorted(rows) == sorted(f"void ionode::ionode_ensemble_step_kernel<{n}>(ionode::EnArgs)" for n in range(1, ion.capi.MCMC_MAX_DIM + 1)), sorted(rows)
    got = {}
    for n in range(1, 14):
        r = rows[f"void ionode::ionode_ensemble_step_kernel<{n}>(ionode::EnArgs)"]
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["agpr"] == 0 and r["lds_static"] == 4, r
        got[n] = r["vgpr"]
    assert got == VGPR, got
    assert max(got.values()) <= 256     # a 256-lane workgroup is one wavefront per SIMD: two ensembles fit a compute unit at every n
