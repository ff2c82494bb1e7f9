"""Training NN-f / NN-d THROUGH the solve: the reference's prediction loss torch.mean(torch.abs(pred_yo - data)) (train-s1.py:329,
train-r1.py:275), which it only watches every 400 iterations (train-r1.py:930-945), minimised with torch.optim.Adam + StepLR on the
gradient the fused objective's backward sweep gives (grad.sum_of_abs / grad.sum_of_squares).

    opt = optim.Adam(func.net.parameters(), lr); scheduler = StepLR(opt, step_size, gamma)
    for itr in range(n_iter):
        loss = mean(|i(odeint(func, y0, t)) - data|);  opt.zero_grad(); loss.backward()
        clip_grad_norm_(func.net.parameters(), max_norm);  opt.step(); scheduler.step()

The weights, Adam's moments, both weight images (the forward solve's and the sweep's) and a small fp64 state block stay in device
memory.  An iteration is the fused forward with checkpoints, the sweep, and three launches of csrc/ionode_train.hpp:
ionode_train_grad_norm (accumulator -> flat fp32 gradient and its norm partials), ionode_train_apply (non-finite guard, norm clip and
Adam, decided on the device) and ionode_train_refresh (both images rebuilt from index maps).  Nothing is packed on the host, no
weight or gradient crosses the bus.

TWO HOST READS REMAIN in an iteration, because they size buffers: the accepted-step count the checkpoint buffer must hold
(grad._forward_with_checkpoints) and the iteration count of the sweep (grad._sweep).  The loop is NOT synchronisation-free.

Because a step may be skipped on the device (a non-finite loss or gradient norm), the host does not know Adam's step count: it
lives in the state block with the bias-correction products.  StepLR counts iterations (the reference calls scheduler.step()
unconditionally); `t`, `report()` and the checkpoint helpers read the block, one small transfer each.
"""
import ctypes as C

import numpy as np
import torch

from . import capi, grad

STATE_DOUBLES = 8
STATE_T, STATE_BETA1_T, STATE_BETA2_T, STATE_SKIPPED, STATE_LOSS, STATE_NORM, STATE_SCALE, STATE_APPLIED = range(8)
MAP_NEG_ZERO, MAP_PLUS_ZERO = -1, -2


def state_dict_floats(L, N):
    return 2 * N + N + L * (N * N + N) + N + 1


def image_maps(mlp_layers, mlp_width):
    """(forward map, grad map) int32 numpy arrays of an (L, N) net for ionode_train_refresh, derived from the library's own packers.
    ionode_mlp_pack of the values 1 .. n gives every element's flat index + 1 and, in the sign bit of its zeros, the -0.0f fill of the
    4-trajectory and one-trajectory sections; ionode_mlp_pack of n times -0.0f is +0.0f exactly where a weight passes through
    "+ 0.0f" (the scalar section's hidden biases).  The grad map is MlpRegression's (0: padding, s > 0: w[s - 1])."""
    L, N = int(mlp_layers), int(mlp_width)
    n = state_dict_floats(L, N)
    if n >= (1 << 24):
        raise capi.IonodeError("index maps go through fp32: the state dict must have fewer than 2^24 floats")
    idx = np.arange(1, n + 1, dtype=np.float32)
    img = capi.mlp_pack(idx, L, N)
    neg = capi.mlp_pack(np.full(n, -0.0, dtype=np.float32), L, N)
    fwd = img.astype(np.int32)
    zero = img == 0.0
    fwd[zero & np.signbit(img)] = MAP_NEG_ZERO
    plus = ~zero & ~np.signbit(neg)
    fwd[plus] = MAP_PLUS_ZERO - (fwd[plus] - 1)
    lib = capi.lib()
    gmap = None
    nimg = lib.ionode_grad_image_floats(L, N)
    if nimg:
        gimg = np.empty(nimg, dtype=np.float32)
        if lib.ionode_grad_pack(idx.ctypes.data, L, N, gimg.ctypes.data) != 0:
            raise capi.IonodeError(lib.ionode_grad_last_error().decode())
        gmap = gimg.astype(np.int32)
    return fwd, gmap


def fresh_state(step=0, beta1=0.9, beta2=0.999):
    """A state block after `step` applied updates: beta^step by `step` multiplications, as the kernel advances them."""
    b1, b2 = np.float64(beta1), np.float64(beta2)
    p1 = p2 = np.float64(1.0)
    for _ in range(int(step)):
        p1, p2 = p1 * b1, p2 * b2
    s = np.zeros(STATE_DOUBLES, dtype=np.float64)
    s[STATE_T], s[STATE_BETA1_T], s[STATE_BETA2_T] = float(step), p1, p2
    return s


class _Ctx:
    """What grad._forward_with_checkpoints saves on an autograd context, outside autograd."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


class ThroughSolve:
    """Trainer state of one net(2 -> N x L -> 1) of NN-f / NN-d and one batch of trajectories, all device-resident.

    model: capi.MODEL_NNF | MODEL_NND; weights_flat [n] fp32 in the reference's state-dict order; params [B, 8] fp64 rate parameters
    (they do not train); protocols_v [P, Np] fp64; data_i [P, Nt] fp64 reference currents; t_eval [Nt] uniform; y0 [B, 2].  N must pad
    to 16, 112, 208 or 512 (the backward sweep's widths; anything else is refused by the library at the first step).
    objective "sae": loss = sum over the succeeded trajectories of sum_k |i_k - data_k| / (n_succeeded * Nt), the reference's
    mean absolute error; "sse": the same with squares.  lr, betas, eps: torch.optim.Adam's; step_size, gamma: StepLR's, counted in
    ITERATIONS; max_norm: clip_grad_norm_'s (0: no clip).  A step whose loss or gradient norm is not finite changes nothing and is
    counted in report()["skipped"].  The remaining keywords are grad.sum_of_abs's.

    evaluate(trainer, lo, hi) -> (loss_sum, count, acc): a stand-in for forward plus sweep over the trajectories [lo, hi): the sum
    of the succeeded trajectories' objective, their number, and the padded fp64 gradient of that SUM (layout:
    ionode_grad_partial_floats) -- tensors on the trainer's device; the trainer divides by count * Nt.  backend="host" keeps the
    state in host memory and runs the library's host mirrors (it needs `evaluate`): with both the loop runs without a GPU.
    group: a torch.distributed group for data-parallel training: every rank solves distributed.shard_bounds' share of the
    trajectories, ONE all-reduce carries [acc | loss sum | count], and every rank applies the identical update.

    Host reads per iteration: two (checkpoint capacity, sweep length), see the module docstring; none for the update."""

    def __init__(self, model, weights_flat, mlp_layers, mlp_width, params, protocols_v, data_i, t_eval, y0, *, objective="sae", lr=1e-3,
                 betas=(0.9, 0.999), eps=1e-8, step_size=100, gamma=0.9, max_norm=0.0, state_dtype=torch.float64, obs_g=1.0, obs_e=-86.0,
                 obs_open_state_only=False, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None, rtol=1e-7, atol=1e-9, v_oob=-80.0,
                 max_steps=0, max_total_steps=0, max_step=0.0, ckpt_cap=None, ckpt_budget_bytes=None, record_budget_bytes=None,
                 evaluate=None, backend="device", group=None, device=None):
        if backend not in ("device", "host"):
            raise capi.IonodeError("backend must be 'device' or 'host'")
        if backend == "host" and evaluate is None:
            raise capi.IonodeError("backend='host' runs the update's host mirrors only: the solve has no CPU path, pass evaluate=")
        if model not in (capi.MODEL_NNF, capi.MODEL_NND):
            raise capi.IonodeError("train.ThroughSolve trains the net of NN-f / NN-d: the closed-form models have no weights")
        if objective not in ("sae", "sse"):
            raise capi.IonodeError("objective must be 'sae' or 'sse'")
        self.host = backend == "host"
        if self.host:
            self.dev = torch.device("cpu")
        else:
            if not torch.cuda.is_available():
                raise capi.IonodeError("no HIP device visible: training through the solve has no CPU fallback")
            self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dev = self.dev
        self.model, self.objective, self.evaluate, self.group = model, objective, evaluate, group
        self.L, self.N = int(mlp_layers), int(mlp_width)
        L, N = self.L, self.N
        lib = capi.lib()
        w = np.ascontiguousarray(np.asarray(weights_flat, dtype=np.float32).reshape(-1))
        self.n = capi.state_dict_floats(w, L, N)
        self.partf = int(lib.ionode_grad_partial_floats(L, N))
        if self.partf == 0:
            raise capi.IonodeError("gradient path needs at least one hidden layer")
        fwd_map, grad_map = image_maps(L, N)
        self.fwd_map, self.grad_map = torch.from_numpy(fwd_map).to(dev), torch.from_numpy(grad_map).to(dev)
        self.fwd_image = torch.empty(fwd_map.size, dtype=torch.float32, device=dev)
        self.grad_image = torch.empty(grad_map.size, dtype=torch.float32, device=dev)
        self.padmap = grad.unpack_partial(torch.arange(self.partf, dtype=torch.float64), L, N).to(torch.int32).to(dev)
        self.w = torch.from_numpy(w.copy()).to(dev)
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.grad = torch.zeros_like(self.w)
        self.norm_part = torch.zeros(int(lib.ionode_train_norm_partials(self.n)), dtype=torch.float64, device=dev)
        self.lr0, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.step_size, self.gamma, self.max_norm = int(step_size), float(gamma), float(max_norm)
        self.itr = 0                                       # iterations run: StepLR's epoch, and which state block is current
        self.state = torch.from_numpy(np.stack([fresh_state(0, *self.betas), np.zeros(STATE_DOUBLES)])).to(dev)
        f64 = lambda t: None if t is None else torch.as_tensor(np.asarray(t) if not isinstance(t, torch.Tensor) else t).to(device=dev, dtype=torch.float64).contiguous()
        self.params, self.prot_v, self.data_i, self.t_eval, self.prot_t = f64(params), f64(protocols_v), f64(data_i), f64(t_eval), f64(prot_t)
        self.y0 = torch.as_tensor(np.asarray(y0) if not isinstance(y0, torch.Tensor) else y0).to(device=dev, dtype=state_dtype).contiguous()
        self.B, self.n_out = int(self.y0.shape[0]), int(self.t_eval.shape[0])
        if self.params.dim() != 2 or self.params.shape[0] != self.B or self.y0.dim() != 2 or self.y0.shape[1] != 2:
            raise capi.IonodeError("params [B, 8] and y0 [B, 2] expected")
        pot = prot_of_traj if prot_of_traj is not None else np.arange(self.B) % int(self.prot_v.shape[0])
        self.prot_of_traj = torch.as_tensor(np.asarray(pot) if not isinstance(pot, torch.Tensor) else pot).to(device=dev, dtype=torch.int32).contiguous()
        self.cfg = None
        if evaluate is None:
            hint = grad.uniform_grid_hint(self.t_eval)
            if hint is None:
                raise capi.IonodeError("train.ThroughSolve needs a uniform output grid t_eval (the fused objective's output cursor)")
            max_step = grad._resolve_max_step(model, self.params, self.prot_v, v_oob, max_step)
            self.cfg = dict(model=model, prot_v=self.prot_v, prot_t=self.prot_t, prot_t0=float(prot_t0), prot_dt=float(prot_dt), t_eval=self.t_eval,
                            rtol=float(rtol), atol=float(atol), v_oob=float(v_oob), max_steps=int(max_steps), max_total_steps=int(max_total_steps),
                            max_step=float(max_step), obs_g=float(obs_g), obs_e=float(obs_e), obs_open_state_only=bool(obs_open_state_only),
                            t_eval_hint=hint, sse_ref=self.data_i, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes, mlp_layers=L,
                            mlp_width=N, weights_key=None, record_budget_bytes=record_budget_bytes, two_phase=True, objective=objective,
                            device_images=(self.fwd_image, self.grad_image))
        self.last = {}          # the last iteration's device tensors: loss, loss_sum, count, status (built-in evaluation)
        self._refresh()

    # ---- plumbing ----
    def _check(self, rc):
        if rc != 0:
            raise capi.IonodeError(capi.lib().ionode_grad_last_error().decode())

    def _call(self, name, *args):
        """The entry point `name` on the current stream, or its _host mirror."""
        lib = capi.lib()
        if self.host:
            self._check(getattr(lib, name + "_host")(*args))
        else:
            self._check(getattr(lib, name)(*args, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))

    def _refresh(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        self._call("ionode_train_refresh", self.n, self.L, self.N, p(self.fwd_map), p(self.grad_map), p(self.w), p(self.fwd_image), p(self.grad_image))

    def lr(self):
        """StepLR: lr0 * gamma ** (iterations // step_size); a skipped step counts (scheduler.step() is unconditional in the reference)."""
        return self.lr0 * self.gamma ** (self.itr // self.step_size)

    # ---- one iteration ----
    def _solve_and_sweep(self, lo, hi, unit_upstream):
        """Forward with checkpoints and sweep over the trajectories [lo, hi) with the resident images: (loss_sum, count, acc), acc the
        gradient of loss_sum (unit_upstream) or of loss_sum / (count * Nt)."""
        cfg = dict(self.cfg, prot_of_traj=self.prot_of_traj[lo:hi].contiguous())
        params, y0 = self.params[lo:hi].contiguous(), self.y0[lo:hi].contiguous()
        ctx = _Ctx()
        r = grad._forward_with_checkpoints(ctx, None, params, y0, cfg, objective=True)
        _params, ckpt, stats, status = ctx.saved_tensors
        per = r[self.objective]
        ok = status == 0
        count = ok.sum().to(torch.float64)
        loss_sum = torch.where(ok, per, torch.zeros_like(per)).sum()
        one = torch.ones((), dtype=torch.float64, device=self.dev)
        up = one if unit_upstream else one / (count * self.n_out)
        g = torch.where(ok, up, torch.zeros_like(up)).contiguous()
        n_acc = torch.where(ok, stats[:, 0], torch.zeros_like(stats[:, 0])).to(torch.int32).contiguous()
        acc, _gp, _gy0 = grad._sweep(cfg, ctx.desc, ctx.w_np, True, params, ckpt, n_acc, g, True)
        self.last.update(status=status, per_trajectory=per)
        return loss_sum, count, acc

    def step(self):
        """One iteration on the current stream.  Returns the loss BEFORE the update as a 0-dim device tensor."""
        lo, hi = 0, self.B
        world = 1
        if self.group is not None:
            import torch.distributed as dist
            from . import distributed
            world = dist.get_world_size(self.group)
            lo, hi = distributed.shard_bounds(self.B, dist.get_rank(self.group), world)
        scaled = False
        if self.evaluate is not None:
            loss_sum, count, acc = self.evaluate(self, lo, hi)
        elif hi > lo:
            scaled = self.group is None    # one rank: the division travels in the upstream gradient, as autograd's would
            loss_sum, count, acc = self._solve_and_sweep(lo, hi, unit_upstream=not scaled)
        else:
            loss_sum, count, acc = 0.0, 0.0, torch.zeros(self.partf, dtype=torch.float64, device=self.dev)
        f64 = lambda x: torch.as_tensor(x, dtype=torch.float64, device=self.dev).reshape(1)
        loss_sum, count = f64(loss_sum), f64(count)
        acc = acc.to(torch.float64).contiguous()
        if self.group is not None:
            import torch.distributed as dist
            bucket = torch.cat([acc, loss_sum, count])
            dist.all_reduce(bucket, op=dist.ReduceOp.SUM, group=self.group)
            acc, loss_sum, count = bucket[:self.partf].contiguous(), bucket[self.partf:self.partf + 1], bucket[self.partf + 1:]
        denom = count * self.n_out
        loss = (loss_sum / denom).contiguous()      # (no succeeded trajectory: 0 / 0, the step is skipped)
        if not scaled:
            acc = acc / denom
        p = lambda t: C.c_void_p(t.data_ptr())
        s_in, s_out = self.state[self.itr & 1], self.state[(self.itr & 1) ^ 1]
        lr = self.lr()
        self._call("ionode_train_grad_norm", self.n, self.L, self.N, p(acc), p(self.padmap), p(self.grad), p(self.norm_part))
        self._call("ionode_train_apply", self.n, self.L, self.N, p(self.grad), p(self.norm_part), p(loss), p(s_in), p(s_out), p(self.w),
                   p(self.m), p(self.v), C.c_float(lr), C.c_double(self.betas[0]), C.c_double(self.betas[1]), C.c_float(self.eps),
                   C.c_double(self.max_norm))
        self.itr += 1
        self._refresh()
        self.last.update(loss=loss, loss_sum=loss_sum, count=count, acc=acc)   # (keeps acc and loss alive until the launches have read them)
        return loss.reshape(())

    def fit(self, n_iter, log_every=0):
        """n_iter iterations; returns the losses at the logged iterations [(itr, lr, loss)] (one read per logged value)."""
        out = []
        for itr in range(n_iter):
            lr = self.lr()
            loss = self.step()
            if log_every and itr % log_every == 0:
                out.append((itr, lr, float(loss.item())))
        return out

    # ---- the state block ----
    def report(self):
        """One read of the state block: applied and skipped steps, and the last iteration's loss, gradient norm and clip scale."""
        s = self.state[self.itr & 1].detach().cpu().numpy()
        return dict(iterations=self.itr, applied=int(s[STATE_T]), skipped=int(s[STATE_SKIPPED]), loss=float(s[STATE_LOSS]),
                    norm=float(s[STATE_NORM]), scale=float(s[STATE_SCALE]), last_applied=bool(s[STATE_APPLIED]), lr=self.lr())

    @property
    def t(self):
        """Adam's step count: the APPLIED updates (one read of the state block; preprocess.adam_state_from_regression reads it)."""
        return int(self.state[self.itr & 1, STATE_T].item())

    def load_adam_state(self, exp_avg, exp_avg_sq, step, iterations=None):
        """Resume: Adam moments in flat state-dict order (preprocess.adam_state_to_flat of a checkpoint's 'optimizer' entry), the
        number of optimiser steps taken and (default: the same) the iterations run, StepLR's epoch."""
        self.m.copy_(torch.as_tensor(np.asarray(exp_avg, dtype=np.float32)).to(self.dev))
        self.v.copy_(torch.as_tensor(np.asarray(exp_avg_sq, dtype=np.float32)).to(self.dev))
        self.itr = int(step if iterations is None else iterations)
        self.state[self.itr & 1].copy_(torch.from_numpy(fresh_state(int(step), *self.betas)).to(self.dev))

    def state_dict_flat(self):
        return self.w.detach().cpu().numpy().copy()
