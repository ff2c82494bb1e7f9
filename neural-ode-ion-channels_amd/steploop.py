"""What the drivers of the four batched optimiser and sampler steps share: fit.py (Levenberg-Marquardt), cmaes.py (CMA-ES), mcmc.py
(adaptive Metropolis), mala.py (manifold MALA) and ensemble.py (the affine-invariant ensemble sampler, which never compacts).  Each of them evaluates a trial tensor of items x rows_per_item trajectories, hands
the result to its step (ionode_<x>_step on the current stream, ionode_<x>_step_host on CPU tensors) and, every compact_every iterations, packs the items
still running into the front launch slots.  The pieces of that are here; the loops stay with the drivers, which differ on purpose in
what comes first (the solve or the step), in how often they run and in when they read the flags.
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def fill_box(d, free, base_params, lo=None, hi=None):
    """The box of a step descriptor (ionode_lm_desc, ionode_cmaes_desc, ionode_mcmc_desc, ionode_mala_desc): free_idx, lo / hi [nf] in the parameters and
    base.  A bound of None is no bound: with d.log_parameters a missing lower bound is the smallest normal number (the steps refuse
    non-positive bounds), else -inf."""
    nf = len(free)
    none_lo = np.finfo(np.float64).tiny if d.log_parameters else -np.inf
    lo = np.full(nf, none_lo) if lo is None else np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.full(nf, np.inf) if hi is None else np.asarray(hi, dtype=np.float64).reshape(-1)
    base = np.asarray(base_params, dtype=np.float64).reshape(-1)
    for j in range(min(nf, capi.LM_MAX_FREE)):
        d.free_idx[j], d.lo[j], d.hi[j] = int(free[j]), float(lo[j]), float(hi[j])
    for i in range(min(base.size, capi.LM_MAX_FREE)):
        d.base[i] = float(base[i])
    return d


def trial_rows(desc, x0, rows_per_item):
    """The initial trial tensor [K * rows_per_item, NPAR] (numpy): every row of item k is the descriptor's base with the free columns
    replaced by x0[k, :nf]."""
    nf = desc.n_free
    params = np.tile(np.array(desc.base[:desc.n_params]), (x0.shape[0], 1))
    params[:, list(desc.free_idx[:nf])] = x0[:, :nf]
    return np.repeat(params, rows_per_item, axis=0)


def step_call(name, desc, dev, want, args):
    """One ionode_<name>_step: `want` lists (name, tensor, dtype, shape) of every tensor that must be a contiguous one on `dev`, `args`
    the tensors (or None) in the entry's argument order behind the descriptor.  On the current stream for device tensors, the host
    mirror ionode_<name>_step_host for CPU tensors."""
    for what, t, dtype, shape in want:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise capi.IonodeError(f"{name}_step: {what}: expected a contiguous {dtype} tensor {shape} on {dev}")
    ptrs = [None if t is None else C.c_void_p(t.data_ptr()) for t in args]
    if dev.type == "cuda":
        rc = getattr(capi.lib(), f"ionode_{name}_step")(C.byref(desc), *ptrs, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    else:
        rc = getattr(capi.lib(), f"ionode_{name}_step_host")(C.byref(desc), *ptrs)
    if rc != 0:
        raise capi.IonodeError(f"ionode_{name}_step failed ({rc}): {capi.lib().ionode_grad_last_error().decode()}")


def problem_tensors(protocols_v, t_eval, data_i, y0, n_traj, state_dtype, dev):
    """(pv [P, Np], te [Nt], ref [P, Nt] fp64, pot [n_traj] int32, y0t [n_traj, D]) on dev for n_traj trajectories laid out item-major,
    protocol-minor: trajectory = (...) * P + protocol."""
    pv = torch.as_tensor(np.asarray(protocols_v), dtype=torch.float64, device=dev).contiguous()
    te = torch.as_tensor(np.asarray(t_eval), dtype=torch.float64, device=dev).contiguous()
    ref = torch.as_tensor(np.asarray(data_i), dtype=torch.float64, device=dev).contiguous()
    P = pv.shape[0]
    pot = torch.from_numpy(np.tile(np.arange(P, dtype=np.int32), n_traj // P)).to(dev)
    y0t = torch.tensor([list(y0)], dtype=state_dtype, device=dev).expand(n_traj, len(y0)).contiguous()
    return pv, te, ref, pot, y0t


def compact(flag, active, n_act, trial, running):
    """The one read of the flags: who is still running.  active: the current slot list (int32 [n_act]) or None (slot = item).  Returns
    the new (active, n_act, trial) -- the items whose flag is `running` packed into the front slots, in ascending order, with their
    rows of trial -- or None when none is left."""
    slots = torch.arange(flag.shape[0], dtype=torch.int32, device=flag.device) if active is None else active
    keep = torch.nonzero(flag[slots.long()] == running).reshape(-1)   # positions among the current slots, ascending
    if keep.numel() == 0:
        return None
    if keep.numel() < n_act:
        npar = trial.shape[1]
        trial = trial.reshape(n_act, -1)[keep].reshape(-1, npar).contiguous()
        active, n_act = slots[keep].to(torch.int32).contiguous(), int(keep.numel())
    return active, n_act, trial


def empty_result(first_shape, dev):
    """What a driver returns for no items at all: (first [0, ...] fp64, value [0] fp64, flag [0] int32, iters [0, 2] int32)."""
    return (torch.zeros((0,) + tuple(first_shape), dtype=torch.float64, device=dev), torch.zeros((0,), dtype=torch.float64, device=dev),
            torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0, 2), dtype=torch.int32, device=dev))
