"""Cases shared by the tests of training through the solve (tests/test_train_host.py, test_train_driver_host.py, test_gpu_train.py).
No GPU needed to import.  The update's cases are drawn: state dicts from (L, N) = (1, 10) upward (n = 151: the 41 floats of N = 10 without
a hidden layer are no case, the gradient path needs one), clip on and off with the
gradient norm on both sides of max_norm, 10 steps each; `run_update` drives ionode_train_grad_norm + ionode_train_apply through
either build, `torch_update` is the reference: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

IMAGE_SHAPES = [(2, 10), (2, 100), (1, 200), (1, 500), (2, 50)]   # scalar section | N = 100 | 4- and one-trajectory sections | N = 500 | generic
UPDATE_SHAPES = [(1, 10), (2, 10), (1, 33), (2, 50), (1, 100)]    # n = 151 .. 10 401: one norm partial and three
N_STEPS = 10
# Relative L2 distance of the weights after 10 steps from torch's clip_grad_norm_ + Adam.  Measured over the 40 cases below (profiles/
# train_through_solve.md): worst 2.476e-8 -- torch forms the norm and the clip factor in fp32 and the bias corrections in Python floats
# from beta ** t, the library the norm in fp64 and the products factor by factor; both round every element-wise operation to fp32.
# Four times the worst case, far inside tests/test_regression.py's FIT_RTOL = 2e-3.
UPDATE_RTOL = 1.0e-7


def n_of(L, N):
    return 2 * N + N + L * (N * N + N) + N + 1


def image_weights(L, N, seed=0):
    """Weights with -0.0f, denormal and negative entries in every tensor."""
    rng = np.random.default_rng(100 * L + N + seed)
    w = rng.normal(0, 0.3, n_of(L, N)).astype(np.float32)
    w[::7] = -0.0
    w[3::11] = np.float32(1e-41)       # denormal
    w[5::13] = -np.float32(3e-42)
    w[1::5] = -np.abs(w[1::5])
    return w


def update_cases():
    out = []
    for k in range(40):
        L, N = UPDATE_SHAPES[k % len(UPDATE_SHAPES)]
        rng = np.random.default_rng(1000 + k)
        n = n_of(L, N)
        gscale = 10.0 ** rng.uniform(-3, 1)
        c = SimpleNamespace(k=k, L=L, N=N, n=n, w=rng.normal(0, 0.3, n).astype(np.float32),
                            grads=(rng.normal(0, gscale, (N_STEPS, n))).astype(np.float32), lr=float(10.0 ** rng.uniform(-4, -2)),
                            betas=(0.9, 0.999), eps=1e-8)
        norm = float(np.linalg.norm(c.grads[0].astype(np.float64)))
        # clip off | the norm far above max_norm | around it (some steps clip, some do not) | far below it
        c.max_norm = [0.0, 0.1 * norm, 1.0 * norm, 10.0 * norm][k % 4]
        out.append(c)
    return out


def padded(ion, g, L, N):
    """A flat gradient scattered into the padded fp64 accumulator layout (what grad._sweep returns), with its flat -> padded map."""
    partf = ion.capi.lib().ionode_grad_partial_floats(L, N)
    padmap = ion.grad.unpack_partial(torch.arange(partf, dtype=torch.float64), L, N).to(torch.int32)
    acc = torch.zeros(partf, dtype=torch.float64)
    acc[padmap.long()] = torch.as_tensor(np.asarray(g, dtype=np.float64))
    return acc, padmap


def run_update(ion, c, grads, losses=None, dev=None, steps=None):
    """N_STEPS of grad_norm + apply through the host mirrors (dev None) or the kernels: (w, m, v, final state block, grad of the last step,
    [state block after every step])."""
    lib = ion.capi.lib()
    train = __import__("importlib").import_module("neural-ode-ion-channels_amd.train")
    host = dev is None
    to = (lambda t: t) if host else (lambda t: t.to(dev))
    w, m, v = to(torch.from_numpy(c.w.copy())), to(torch.zeros(c.n)), to(torch.zeros(c.n))
    grad = to(torch.zeros(c.n))
    _, padmap = padded(ion, grads[0], c.L, c.N)
    padmap = to(padmap)
    part = to(torch.zeros(lib.ionode_train_norm_partials(c.n), dtype=torch.float64))
    state = to(torch.from_numpy(np.stack([train.fresh_state(0, *c.betas), np.zeros(8)])))
    p = lambda t: C.c_void_p(t.data_ptr())
    tail = [] if host else [C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)]
    sfx = "_host" if host else ""
    blocks, keep = [], []
    for it in range(len(grads) if steps is None else steps):
        acc = to(padded(ion, grads[it], c.L, c.N)[0])
        loss = to(torch.tensor([1.0 if losses is None else losses[it]], dtype=torch.float64))
        keep += [acc, loss]
        rc = getattr(lib, "ionode_train_grad_norm" + sfx)(c.n, c.L, c.N, p(acc), p(padmap), p(grad), p(part), *tail)
        assert rc == 0, lib.ionode_grad_last_error()
        rc = getattr(lib, "ionode_train_apply" + sfx)(c.n, c.L, c.N, p(grad), p(part), p(loss), p(state[it & 1]), p(state[(it & 1) ^ 1]), p(w),
                                                    p(m), p(v), c.lr, c.betas[0], c.betas[1], c.eps, c.max_norm, *tail)
        assert rc == 0, lib.ionode_grad_last_error()
        blocks.append(state[(it & 1) ^ 1].cpu().numpy().copy())
    np_ = lambda t: t.cpu().numpy().copy()
    return np_(w), np_(m), np_(v), blocks[-1], np_(grad), blocks


def torch_update(c, grads):
    wt = torch.from_numpy(c.w.copy()).requires_grad_(True)
    opt = torch.optim.Adam([wt], lr=c.lr, betas=c.betas, eps=c.eps)
    scales = []
    for g in grads:
        wt.grad = torch.from_numpy(g.copy())
        if c.max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([wt], c.max_norm)
            scales.append(min(1.0, c.max_norm / (float(total) + 1e-6)))
        opt.step()
    return wt.detach().numpy().copy(), scales


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
