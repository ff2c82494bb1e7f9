"""Code-object hygiene of the manifold-MALA step kernels (no GPU): register, scratch and LDS figures read from the library's metadata
notes with tools/kernel_resources.py, as tests/test_mcmc_kernel_resources.py does for the adaptive-Metropolis step.  One lane per
chain keeps ONE packed lower triangle in registers -- 91 words at 13 coordinates, the trial's factor through the tell and then, word
by word, the chain's own for the proposal -- and nothing in scratch or LDS (LDS is zero: the stated formula); the register figures of
the build that ships are pinned (a compiler that changes them should be looked at)."""
import importlib
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

# n: registers a lane holds (architectural and accumulation registers together), of the shipped build
VGPR = {1: 48, 2: 64, 3: 77, 4: 98, 5: 116, 6: 141, 7: 168, 8: 192, 9: 227, 10: 250, 11: 282, 12: 325, 13: 368}
# n: values the allocator parks in free accumulation registers (register-to-register copies: no scratch); none up to n = 11
AGPR_PARKED = {12: 48, 13: 64}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_step_kernels_use_no_scratch_and_no_lds_and_their_registers_are_pinned():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    from kernel_resources import kernel_resources
    rows = {r["kernel"]: r for r in kernel_resources(ion.capi.LIB_PATH) if "ionode_mala_step_kernel<" in r["kernel"]}
    assert sorted(rows) == sorted(f"void ionode::ionode_mala_step_kernel<{n}>(ionode::MaArgs)" for n in range(1, ion.capi.MCMC_MAX_DIM + 1)), sorted(rows)
    got, parked = {}, {}
    for n in range(1, 14):
        r = rows[f"void ionode::ionode_mala_step_kernel<{n}>(ionode::MaArgs)"]
        assert r["scratch_bytes"] == 0 and r["lds_static"] == 0 and r["vgpr"] <= 512, r
        got[n] = r["vgpr"]
        if r["vgpr_spill"]:
            parked[n] = r["vgpr_spill"]
    assert got == VGPR, got
    assert parked == AGPR_PARKED, parked
    assert got[5] <= 128     # p1 .. p4 and sigma, the benchmark's case: four wavefronts per SIMD
