"""Trajectory sharding across the GPUs of one node and the path's only collective.

Trajectories are independent (each `odeint` call of the reference is its own solve, e.g. train-s1.py:566-580), so
the batch index is cut into contiguous shards, one process per GPU, and the forward solve needs no data-path
collective.  An objective evaluation (mean |i_pred - i_ref| as train-s1.py:329, or a sum of squares as
train-d0.py:508-540) reduces two fp64 scalars with ONE all-reduce -- RCCL over xGMI when the process group is
`nccl`, gloo on CPU in the tests.
"""
import os

import torch


def env_rank_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def shard_bounds(n, rank, world):
    """Contiguous [lo, hi) of `n` items for `rank`; the first n % world ranks get one extra item."""
    if not (0 <= rank < world):
        raise ValueError("rank outside world")
    base, extra = divmod(n, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_bounds_by_cost(cost, world):
    """Contiguous shards of equal predicted COST instead of equal count: [(lo, hi)] * world, covering range(len(cost)).

    Solves differ 2-3x in step count, so equal counts leave the ranks with the easy candidates idle at the
    all-reduce.  cost: per-item prediction (the previous evaluation's RHS-evaluation counts, schedule.pilot_cost(), ...);
    the cut after rank r is placed where the running sum first reaches (r + 1) / world of the total.  Every rank computes
    the same cuts from the same `cost`, so no communication is needed; zero or non-finite costs fall back to equal counts."""
    import numpy as np
    c = np.asarray(cost.detach().cpu() if isinstance(cost, torch.Tensor) else cost, dtype=np.float64).reshape(-1)
    n = c.size
    if world < 1:
        raise ValueError("world must be positive")
    if n == 0 or not np.isfinite(c).all() or (c < 0).any() or c.sum() <= 0:
        return [shard_bounds(n, r, world) for r in range(world)]
    cum = np.cumsum(c)
    cuts = [0]
    for r in range(1, world):
        k = int(np.searchsorted(cum, cum[-1] * r / world, side="left")) + 1   # first prefix reaching r/world of the total
        cuts.append(min(max(k, cuts[-1]), n))
    cuts.append(n)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def population_shards(n, cost, group=None, noun="candidates"):
    """(rank, world, bounds) of a population of n items cut over the group's ranks: bounds [(lo, hi)] * world, contiguous, of equal
    count or -- with cost [n] -- of equal predicted cost (shard_bounds_by_cost).  (0, 1, [(0, n)]) outside torch.distributed."""
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
    if cost is not None and len(cost) != n:
        from .capi import IonodeError
        raise IonodeError(f"cost has {len(cost)} entries for {n} {noun}: the shards would not cover the population")
    bounds = [shard_bounds(n, r, world) for r in range(world)] if cost is None else shard_bounds_by_cost(cost, world)
    return rank, world, bounds


def all_gather_shards(out, bounds, rank, group=None):
    """The whole population's rows from every rank's out [hi - lo, ...] (its shard bounds[rank]): one all-gather of the shards padded
    to the largest, the padding cut away again.  World size 1: out itself."""
    import torch.distributed as dist
    world = len(bounds)
    if world == 1:
        return out
    m = max(hi - lo for lo, hi in bounds)
    pad = torch.full((m,) + tuple(out.shape[1:]), float("inf"), dtype=out.dtype, device=out.device)
    pad[: bounds[rank][1] - bounds[rank][0]] = out
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    return torch.cat([parts[r][: hi - lo] for r, (lo, hi) in enumerate(bounds)])


def init_process_group(backend=None, device=None):
    """One process per GPU; nccl (= RCCL) when a HIP device is given, gloo otherwise.  No-op for world size 1."""
    import torch.distributed as dist
    rank, world, local = env_rank_world()
    if world == 1 or dist.is_initialized():
        return dist if dist.is_initialized() else None
    if backend is None:
        backend = "nccl" if (device is not None and torch.device(device).type == "cuda") else "gloo"
    kw = {"device_id": torch.device(device)} if backend == "nccl" and device is not None else {}
    dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    return dist


def allreduce_sum_count(total, count, group=None):
    """Sum a (sum, count) pair over all ranks with one all-reduce; returns (global_sum, global_count) tensors."""
    import torch.distributed as dist
    pair = torch.stack([torch.as_tensor(total, dtype=torch.float64).reshape(()),
                        torch.as_tensor(float(count), dtype=torch.float64, device=torch.as_tensor(total).device).reshape(())])
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(pair, op=dist.ReduceOp.SUM, group=group)
    return pair[0], pair[1]


def sharded_mean_abs_loss(solve_shard, i_ref, n_traj, group=None):
    """Global mean |i_pred - i_ref| over `n_traj` trajectories sharded over the ranks.

    solve_shard(lo, hi) -> [hi - lo, Nt] current traces of this rank's trajectories (a torch tensor on the rank's
    device); i_ref: the matching [hi - lo, Nt] reference slice or a callable (lo, hi) -> tensor.
    """
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    lo, hi = shard_bounds(n_traj, rank, world)
    pred = solve_shard(lo, hi)
    ref = i_ref(lo, hi) if callable(i_ref) else i_ref
    ref = torch.as_tensor(ref, dtype=pred.dtype, device=pred.device)
    s, c = allreduce_sum_count((pred - ref).abs().sum(), pred.numel(), group=group)
    return s / c


def sharded_mean_abs_loss_fused(solve_shard, n_traj, n_out, group=None):
    """sharded_mean_abs_loss without the traces: the global mean |i_pred - i_ref| over `n_traj` trajectories of `n_out` samples each.

    solve_shard(lo, hi) -> [hi - lo] fused sums of absolute residuals of this rank's trajectories (Solution.sae of a solve with
    sse_ref and objective="sae": the reference currents never leave the kernel's side).  One allreduce_sum_count of
    (sum, (hi - lo) * n_out) follows.  A failed trajectory's inf makes the mean inf.
    """
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    lo, hi = shard_bounds(n_traj, rank, world)
    sae = solve_shard(lo, hi)
    if tuple(sae.shape) != (hi - lo,):
        raise ValueError(f"solve_shard({lo}, {hi}) returned shape {tuple(sae.shape)}, expected {(hi - lo,)}")
    s, c = allreduce_sum_count(sae.sum(), (hi - lo) * n_out, group=group)
    return s / c


def sharded_mean_abs_loss_fused_s1(solve_shard, leaves, n_traj, n_out, group=None):
    """sharded_mean_abs_loss_fused WITH its gradient: (loss, [dloss/dleaf for leaf in leaves]), the reference's training loss
    torch.mean(torch.abs(pred_yo - data)) (train-s1.py:329) over `n_traj` trajectories of `n_out` samples sharded over the ranks.

    solve_shard(lo, hi) -> this rank's DIFFERENTIABLE [hi - lo] fused sums of absolute residuals (grad.sum_of_abs), whose graph
    reaches `leaves` (tensors that require grad and that every rank holds whole: shared weights, shared rate parameters).  The global
    mean comes from one allreduce_sum_count; the rank's share sum(sae) / (n_traj * n_out) is backpropagated, and the leaves' gradients
    are summed over the ranks with grad.allreduce_gradients, one bucket.  A leaf the rank's shard does not reach (an empty shard)
    contributes zeros.  A failed trajectory's inf makes the loss inf; its gradient rows are zero (grad.sum_of_abs).
    """
    import torch.distributed as dist
    from . import grad
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    lo, hi = shard_bounds(n_traj, rank, world)
    sae = solve_shard(lo, hi)
    if tuple(sae.shape) != (hi - lo,):
        raise ValueError(f"solve_shard({lo}, {hi}) returned shape {tuple(sae.shape)}, expected {(hi - lo,)}")
    s, c = allreduce_sum_count(sae.detach().sum(), (hi - lo) * n_out, group=group)
    leaves = list(leaves)
    grads = [None] * len(leaves)
    if hi > lo and sae.requires_grad:
        grads = torch.autograd.grad(sae.sum() / float(n_traj * n_out), leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if g is None else g for leaf, g in zip(leaves, grads)]
    return s / c, grad.allreduce_gradients(grads, group=group)
