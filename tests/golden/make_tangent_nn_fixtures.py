"""Writes tests/golden/tangent_nn_jacobians.npz: the checker's Jacobians (tests/tangent_nn_check.py `jacobian`: forward-mode AD through
the torch replay of the oracle's accepted steps, with the weights) of the cases tests/test_gpu_tangent_nn.py compares the HIP sweep
with.  Recorded because one forward-mode pass through the replay takes 1.5 s on a CPU (torch's dual numbers times Python scalars) and
a case needs 7 trajectories x 8 parameters of them; tests/test_tangent_nn_host.py recomputes one trajectory against the record and
checks every recorded row against the step algebra written out by hand.  No GPU needed.

    python tests/golden/make_tangent_nn_fixtures.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import sse_nn_cases as N   # noqa: E402
import tangent_nn_check as T   # noqa: E402
from oracle import oracle   # noqa: E402


def main():
    oracle.build()
    torch.set_num_threads(1)
    out = {}
    for L, N_, model in T.CASES:
        for f32 in (False, True):
            c = N.problem(L, N_, model, f32)
            rows = T.checked_rows(c)
            out[T.case_key(L, N_, model, f32)] = np.stack([T.jacobian(oracle, c, b)[1] for b in rows])
            print(T.case_key(L, N_, model, f32), rows, out[T.case_key(L, N_, model, f32)].shape, flush=True)
    np.savez_compressed(os.path.join(HERE, "tangent_nn_jacobians.npz"), **out)


if __name__ == "__main__":
    main()
