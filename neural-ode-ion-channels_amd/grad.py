"""Gradients through the batched solve (BASELINE.json configs[4]).

Reference interface: `from torchdiffeq import odeint_adjoint as odeint` (train-s1.py:29-32).  The reference only switches
that import -- every call site runs under torch.no_grad() and nothing is ever differentiated (SURVEY.md finding 3) -- so
there is no reference gradient to reproduce: **parity is unpinned**.  What this module computes is the exact reverse-mode
derivative of the discretisation the forward launch executed, with the accepted steps (t0, dt) as constants
(discretise-then-optimise, controller frozen); the checker is autograd through a torch restatement replaying the same
steps (tests/grad_check.py).  `odeint` and `odeint_adjoint` share this backward: both names give the same values and the
same gradients.

Three launches per backward (csrc/ionode_grad.hpp, ionode_grad_reduce.hpp), all through the C ABI:
  forward   ionode_dopri5 with accepted-step checkpoints (160 B per step and trajectory)
  sweep     adjoints of y0 and p1..p8, and the (d_l, h_l) record stream of every MLP vector-Jacobian product (160 KB per
            16-trajectory tile evaluation for s00 -- sized for 288 GB of HBM3E and chunked over iterations above
            `record_budget_bytes`).  NN models: two phases -- ionode_dopri5_backward_recompute (unit-seed products of every
            (tile, step) at once, whole chip) one chunk ahead of ionode_dopri5_backward_sweep (the sequential walk: adjoint
            algebra only); closed-form models and two_phase=False: ionode_dopri5_backward (everything inside the walk)
  reduce    ionode_grad_reduce[_unit]: split-K fp32 MFMA GEMM of the records into per-slab partial weight gradients, summed
            here in fp64.
sum_of_squares: the fused objective sse[b] = sum_k (i_k - ref_k)^2 with its gradient, nothing of size [B, Nt] allocated.  Closed-form
models: the one-phase sweep with the seed formed in the kernel (ionode_dopri5_backward_sse).  NN models: the two-phase sweep above
without grad_y -- ionode_dopri5_backward_sse_gc (csrc/ionode_grad_gc.hpp) forms each chunk's interpolant-coefficient adjoints and the
sample-0 term, ionode_dopri5_backward_recompute_sse / _sweep_sse are the recompute and walk launches that take them.
sum_of_abs: the same with sae[b] = sum_k |i_k - ref_k|, Nt times the reference's loss torch.mean(torch.abs(pred_yo - data)) (train-s1.py:329,
train-d1.py:305, train-r1.py:275) -- the same forward (objective="sae"), the same launches: the kind travels in cfg["objective"] to
ionode_objective_backward / ionode_objective_backward_gc (capi.OBJECTIVE_BUFFERS), the two entry points that form the residuals'
weights (2 g r or g sign(r)) and with the squares' kind ARE _sse / _sse_gc; the recompute, the walk and the reduce never see a residual.
Both routes are one autograd Function each (_Solve, _FusedObjective) over the same three pieces: _forward_with_checkpoints, _backward
(failed trajectories masked, rows zeroed) and the chunk loop _sweep, which calls the sweep entry points through capi.sweep_launch /
capi.objective_launch with every buffer named (capi.SWEEP_BUFFERS, capi.OBJECTIVE_BUFFERS).
There is no CPU fallback: without libionode.so or a HIP device every call raises.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import capi

_image_cache = {}
DEFAULT_CKPT_CAP = 4096
DEFAULT_RECORD_BUDGET = 64 << 30   # of 288 GB HBM3E per GPU: two record buffers of half of it (24 GB: +1.5 % sweep time; 96 GB: -0.5 %)
DEFAULT_CKPT_BUDGET = 96 << 30   # bytes of accepted-step checkpoints one forward may allocate (a third of the 288 GB of HBM3E)
MAX_RECOMPUTE_ITERS = 65535 * 4  # phase A launches dim3(tiles, ceil(iterations / GRAD_RECOMPUTE_IB = 4)): HIP caps grid.y at 65535
RESIDENT_IMAGES = "resident"      # what stands for the host weights when cfg["device_images"] = (forward image, grad image) hands both in


def _bounded_budget(requested, default, dev, share):
    """An explicit budget is taken as given; the default (tuned for an empty 288 GB MI355X) is capped at `share` of the memory
    that is free on `dev` right now, so that a smaller or partly occupied GPU gets smaller chunks instead of an allocator failure."""
    if requested:
        return int(requested)
    try:
        free, _total = torch.cuda.mem_get_info(dev)
        # memory the caching allocator holds but has handed out to nobody is reusable by the next allocation: without it the previous
        # iteration's own freed checkpoint / record buffers would shrink the budget iteration by iteration
        free += max(0, torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
    except Exception:  # no device query available: keep the default
        return int(default)
    return int(max(1 << 28, min(default, share * free)))


def stable_step_cap(model, params, prot_v, v_oob=-80.0, safety=3.0):
    """Largest dt (ms) that keeps dopri5 inside its real-axis stability interval (|h lambda| < ~3.3) for every trajectory
    of the batch: safety / lambda_max, lambda_max = the largest relaxation rate of the gating equations at the protocol's
    extreme voltages (the rates p exp(+-q v) are monotone in v, so the maximum sits at an end of the voltage range).
    2-state models: lambda = k_open + k_close of the a and r gates (train-s1.py:161-177); 6-state model: Gershgorin bound
    2 x (sum of the six rates) (train-d1.py:165-187).  This is what `max_step="auto"` passes to the solve."""
    p = params.detach().to(torch.float64)
    v = torch.stack([prot_v.min().to(torch.float64), prot_v.max().to(torch.float64),
                     torch.as_tensor(float(v_oob), dtype=torch.float64, device=prot_v.device)]).to(p.device)
    n = 6 if model == capi.MODEL_MARKOV6 else 4
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(n)], dtype=torch.float64, device=p.device)
    amp, exp = p[:, 0:2 * n:2], p[:, 1:2 * n:2] * sign            # [B, n]
    rates = amp[:, :, None] * torch.exp(exp[:, :, None] * v[None, None, :])   # [B, n, 3]
    if model == capi.MODEL_MARKOV6:
        lam = 2.0 * rates.abs().sum(1)
    else:
        pairs = rates.abs().reshape(p.shape[0], n // 2, 2, 3).sum(2)          # (k1 + k2), (k3 + k4)
        if model == capi.MODEL_NNF:
            pairs = pairs[:, 1:]                                              # the a gate is the MLP: only the r gate is stiff
        lam = pairs.amax(1)
    lam_max = float(lam.max().item())
    return safety / lam_max if lam_max > 0 and np.isfinite(lam_max) else 0.0


def _forward_with_checkpoints(ctx, weights_flat, params, y0, cfg, objective):
    """The forward of both autograd Functions: capi.dopri5 with the packed image of weights_flat (None: a closed-form model), cfg's
    keywords and accepted-step checkpoints; objective: the fused objective of kind cfg["objective"] (sse_ref, obs_*; no state trace) instead of the states.
    cfg["device_images"] = (forward image, grad image),
    two device tensors (optional): the images the launches read, instead of packing and uploading weights_flat (then None) -- _sweep reads the second.
    The [B, cap, record] checkpoint buffer is sized by ckpt_cap / ckpt_budget_bytes and regrown (the forward runs again) until the steps
    of every trajectory that SUCCEEDED fit.  Saves what _backward reads on ctx and returns capi.dopri5's result."""
    dev = y0.device
    B, D = y0.shape
    L, N = cfg["mlp_layers"], cfg["mlp_width"]
    w_np, packed = None, None
    if cfg.get("device_images") is not None:   # (train.ThroughSolve: both images already lie in device memory; nothing is packed or uploaded)
        w_np, packed = RESIDENT_IMAGES, cfg["device_images"][0]
    elif weights_flat is not None:
        w_np = weights_flat.detach().to(torch.float32).cpu().numpy()
        from . import batched  # packed forward image: shared cache with the plain solve
        packed = batched.packed_weights(w_np, L, N, dev, key=cfg.get("weights_key"))
    kw = dict(mlp_packed=packed, mlp_layers=L, mlp_width=N, prot_t=cfg.get("prot_t"), prot_t0=cfg["prot_t0"], prot_dt=cfg["prot_dt"],
              prot_of_traj=cfg.get("prot_of_traj"), rtol=cfg["rtol"], atol=cfg["atol"], v_oob=cfg["v_oob"], max_steps=cfg["max_steps"],
              max_total_steps=cfg["max_total_steps"], max_step=cfg.get("max_step", 0.0), tile_waves=cfg.get("tile_waves", 0),
              t_eval_hint=cfg.get("t_eval_hint", "auto"))
    if objective:
        kw.update(obs_g=cfg["obs_g"], obs_e=cfg["obs_e"], obs_open_state_only=cfg["obs_open_state_only"], sse_ref=cfg["sse_ref"], states=False,
                  objective=cfg["objective"])
    kw.update(cfg.get("forward_kw") or {})   # (sensitivity.current_s1: the current epilogue beside the states)
    cap = int(cfg.get("ckpt_cap") or DEFAULT_CKPT_CAP)
    limit = _bounded_budget(cfg.get("ckpt_budget_bytes"), DEFAULT_CKPT_BUDGET, dev, 0.6)
    row_bytes = B * capi.ckpt_record_doubles(D) * 8
    if cap * row_bytes > limit:   # the FIRST allocation obeys the budget too (a huge batch on a small or occupied GPU)
        cap = max(1, limit // row_bytes)
    while True:
        ckpt = None   # (a regrown buffer replaces the old one instead of coexisting with it)
        ckpt = torch.empty((B, cap, capi.ckpt_record_doubles(D)), dtype=torch.float64, device=dev)
        r = capi.dopri5(cfg["model"], params.detach(), cfg["prot_v"], y0.detach(), cfg["t_eval"], ckpt=ckpt, **kw)
        # the checkpoint buffer is sized for the trajectories that SUCCEEDED: a failed one (status != 0: step budget spent,
        # dt underflow) can have 10^5..10^6 accepted steps, contributes no gradient (its n_acc is zeroed in backward) and
        # must not grow a [B, cap, record] buffer to hundreds of GB
        nacc = torch.where(r["status"] == 0, r["stats"][:, 0], torch.zeros_like(r["stats"][:, 0]))
        most = int(nacc.max().item())
        if most <= cap:
            break
        cap = 1 << int(np.ceil(np.log2(most + 1)))  # the buffer was too small: run the forward again with room
        if cap * row_bytes > limit and most * row_bytes <= limit:
            cap = limit // row_bytes   # the power of two does not fit the budget, the steps themselves do
        need = cap * row_bytes
        if need > limit:
            raise capi.IonodeError(f"checkpoints of {most} accepted steps x {B} trajectories need {need / 2**30:.1f} GiB "
                                   f"(> ckpt_budget_bytes = {limit / 2**30:.1f} GiB): split the batch or raise the budget")
    ctx.cfg, ctx.desc, ctx.w_np = cfg, r["desc"], w_np
    ctx.vtab = r["v_at_outputs"]   # (when the descriptor points at one, the backward reads V(t_k) from the same table)
    ctx.save_for_backward(params.detach(), ckpt, r["stats"], r["status"])
    ctx.mark_non_differentiable(r["status"])
    return r


def plan_backward_chunks(n_iter, tiles, record_floats, packet_doubles, budget, need_w, two_phase):
    """How _sweep cuts the n_iter sweep iterations into launches: (chunk, n_buf, bounds) -- iterations per chunk, buffer
    pairs (2: the next chunk is produced while this one is reduced / walked), and the chunks' [it0, it1) ranges.  Pure arithmetic
    (tests/test_host_logic.py replays tests/golden/grad_chunk_plans.json through it).
      with weight gradients   a chunk's record stream (6 records of record_floats fp32 per tile and iteration) fits the budget; once
                              that takes more than one chunk there are two buffers of half the budget each
      two-phase without them  the packets (packet_doubles fp64 per tile and iteration) are what a chunk holds: two buffers, at most
                              256 iterations each, which also keeps phase A one chunk ahead
      otherwise               one launch
    Two-phase chunks stay inside MAX_RECOMPUTE_ITERS (HIP's grid.y limit for phase A)."""
    most = min(n_iter, MAX_RECOMPUTE_ITERS) if two_phase else n_iter
    if need_w:
        per_it = tiles * 6 * record_floats * 4
        chunk = max(1, min(most, budget // per_it))
        if chunk < n_iter:
            chunk = max(1, min(most, (budget // 2) // per_it))
    elif two_phase:
        chunk = max(1, min(most, 256, (budget // 2) // (tiles * packet_doubles * 8)))
    else:
        chunk = n_iter
    n_buf = 2 if chunk < n_iter and (need_w or two_phase) else 1
    return chunk, n_buf, [(it0, min(n_iter, it0 + chunk)) for it0 in range(0, n_iter, chunk)]


def _resolve_max_step(model, params, prot_v, v_oob, max_step, frames=2):
    """max_step of solve / sum_of_squares / sum_of_abs as a number: "auto" = stable_step_cap(); warns (at the user's call: `frames`
    frames up) when the rate parameters require grad and no cap is set."""
    if isinstance(max_step, str):
        if max_step != "auto":
            raise capi.IonodeError("max_step must be a number (ms) or 'auto'")
        return stable_step_cap(model, params, prot_v, v_oob)
    if float(max_step) == 0.0 and isinstance(params, torch.Tensor) and params.requires_grad:
        import warnings
        warnings.warn("gradients w.r.t. the rate parameters through an UNCAPPED dopri5 solve: at equilibria dopri5 accepts steps with "
                      "h*lambda >> 1 whose exact derivative amplifies rounding noise without bound (|dL/dp| ~ 1e36 on long holds, "
                      "DESIGN.md 5.4).  Pass max_step='auto' (= 3 / lambda_max of the rate constants, grad.stable_step_cap) or a "
                      "value in ms; the forward values then follow the capped step sequence.", RuntimeWarning, stacklevel=frames + 1)
    return max_step


def grad_image(weights_flat, L, N, dev, key=None):
    """Device-resident grad image (forward + transposed MFMA fragments) of a flat fp32 state dict."""
    ck = (key, L, N, str(dev)) if key is not None else None
    if ck is not None and ck in _image_cache:
        return _image_cache[ck]
    w = np.ascontiguousarray(np.asarray(weights_flat, dtype=np.float32).reshape(-1))
    capi.state_dict_floats(w, L, N)
    n = capi.lib().ionode_grad_image_floats(L, N)
    if n == 0:
        raise capi.IonodeError("gradient path needs at least one hidden layer")
    out = np.empty(n, dtype=np.float32)
    if capi.lib().ionode_grad_pack(w.ctypes.data, L, N, out.ctypes.data) != 0:
        raise capi.IonodeError(capi.lib().ionode_grad_last_error().decode())
    img = torch.from_numpy(out).to(dev)
    if ck is not None:
        if len(_image_cache) > 8:
            _image_cache.clear()
        _image_cache[ck] = img
    return img


def unpack_partial(part, L, N):
    """Padded partial-gradient layout (include/ionode.h: ionode_grad_partial_floats) -> flat state-dict order."""
    NP = 16 * ((N + 15) // 16)
    out = []
    j0 = part[:4 * NP].reshape(NP, 4)
    out += [j0[:N, 1:3].reshape(-1), j0[:N, 0]]
    off = 4 * NP
    for _ in range(L):
        W = part[off:off + NP * NP].reshape(NP, NP)
        b = part[off + NP * NP:off + NP * NP + NP]
        out += [W[:N, :N].reshape(-1), b[:N]]
        off += NP * NP + NP
    out += [part[off:off + N], part[off + NP:off + NP + 1]]
    return torch.cat(out)


class _Solve(torch.autograd.Function):
    """y[B, Nt, D] = dopri5 solve; differentiable in (weights_flat, params, y0)."""

    @staticmethod
    def forward(ctx, weights_flat, params, y0, cfg):
        r = _forward_with_checkpoints(ctx, weights_flat, params, y0, cfg, objective=False)
        return r["y"], r["status"]

    @staticmethod
    def backward(ctx, gy, _gstatus):
        return _backward(ctx, gy, fused=False)


class _FusedObjective(torch.autograd.Function):
    """The fused forward's per-trajectory sums [B] of kind cfg["objective"]: "sse", sum_k (i_k - sse_ref[protocol][k])^2, or "sae",
    sum_k |i_k - sse_ref[protocol][k]|; differentiable in (weights_flat, params, y0).  Nothing of size [B, Nt] is ever allocated: the
    forward writes checkpoints and sse_out (no state trace), the backward sweeps with the [B] upstream gradient."""

    @staticmethod
    def forward(ctx, weights_flat, params, y0, cfg):
        r = _forward_with_checkpoints(ctx, weights_flat, params, y0, cfg, objective=True)
        return r[cfg["objective"]], r["status"]

    @staticmethod
    def backward(ctx, g_sse, _gstatus):
        return _backward(ctx, g_sse, fused=True)


def _backward(ctx, g, fused):
    """The backward of both Functions: g is the upstream dL/dy [B, Nt, D], or (fused) dL/dsum [B].  Failed trajectories (status != 0:
    their rows of y are NaN-filled, their sum is inf) carry no gradient: their upstream rows are zeroed (a caller's unmasked loss would
    otherwise feed NaN into the sweep), they replay no steps, and their rows of dL/dp and dL/dy0 are zero."""
    cfg, desc = ctx.cfg, ctx.desc
    params, ckpt, stats, status = ctx.saved_tensors
    sdt = torch.float32 if desc.state_f32 else torch.float64
    failed = status != 0
    g = torch.where(failed.reshape((-1,) + (1,) * (g.dim() - 1)), torch.zeros((), dtype=g.dtype, device=g.device), g)
    g = g.to(torch.float64 if fused else sdt).contiguous()
    n_acc = torch.where(failed, torch.zeros_like(stats[:, 0]), stats[:, 0]).to(torch.int32).contiguous()
    need_w = ctx.needs_input_grad[0] and ctx.w_np is not None
    acc, g_params, g_y0 = _sweep(cfg, desc, ctx.w_np, need_w, params, ckpt, n_acc, g, fused)
    g_params[failed] = 0.0
    g_y0[failed] = 0.0
    g_w = unpack_partial(acc, cfg["mlp_layers"], cfg["mlp_width"]).to(torch.float32) if need_w else None
    return g_w, (g_params if ctx.needs_input_grad[1] else None), (g_y0.to(sdt) if ctx.needs_input_grad[2] else None), None


def _sweep(cfg, desc, w_np, need_w, params, ckpt, n_acc, g, fused):
    """The backward sweep's chunk loop.  g: the upstream dL/dy [B, Nt, D] in the state dtype, or (fused) dL/dsum [B] fp64 of the
    fused objective of kind cfg["objective"] -- closed-form models: one launch of ionode_objective_backward; NN models: two-phase only,
    per chunk ionode_objective_backward_gc forms the packets' G_c on the phase-A stream and the products run without grad_y.  n_acc [B] int32:
    accepted steps to replay (0 for failed trajectories).  Returns (padded partial weight gradient fp64 | None, dL/dp [B, NPAR], dL/dy0
    [B, D]), the rows of failed trajectories not yet zeroed."""
    dev = params.device
    L, N = cfg["mlp_layers"], cfg["mlp_width"]
    B = desc.n_traj
    lib = capi.lib()
    # Two-phase sweep (NN models; csrc/ionode_grad.hpp).  A stage's vector-Jacobian product is linear in its seed
    # (a scalar per trajectory) and everything else it needs comes from the step's checkpoint: phase A
    # (ionode_dopri5_backward_recompute) computes the UNIT-SEED products of every (tile, step) of a chunk at once on the whole
    # chip, on its own stream, one chunk AHEAD of phase B (ionode_dopri5_backward_sweep: the sequential walk, adjoint algebra
    # only, one wavefront per tile); the reduction of a finished chunk (ionode_grad_reduce_unit: records scaled by the seeds
    # the walk wrote) runs on a third stream.  Records and packets are double-buffered.
    two_phase = bool(cfg.get("two_phase", os.environ.get("IONODE_GRAD_ONE_PHASE", "0") != "1")) and w_np is not None
    if fused and w_np is not None and not two_phase:
        raise capi.IonodeError("the fused objective's sweep of the NN models is two-phase only: use grad.solve for the one-phase sweep")
    desc.ckpt, desc.ckpt_cap = ckpt.data_ptr(), ckpt.shape[1]
    gc_desc = desc
    if fused and two_phase and desc.v_at_outputs is None and 4 * desc.n_prot <= desc.n_traj:
        # V(t_k) once per protocol ([P, Nt]) instead of one lookup per trajectory and sample: capi.dopri5's "auto" rule for the
        # closed-form epilogue, here for the G_c launches alone (the NN forward has formed its own voltages already), which get a
        # descriptor of their own that points at the table; it lives for this sweep
        vtab = capi.protocol_at_outputs(desc, cfg["prot_v"], cfg.get("prot_t"), cfg["t_eval"])
        gc_desc = capi.IonodeDesc.from_buffer_copy(desc)
        gc_desc.v_at_outputs = vtab.data_ptr()
    n_iter = int(n_acc.max().item()) + 1
    if cfg.get("device_images") is not None:
        image = cfg["device_images"][1]
    else:
        image = grad_image(w_np, L, N, dev, key=cfg.get("weights_key")) if w_np is not None else None
    D, npar = desc.n_state, capi.n_params(desc.model)
    state = torch.empty((B, 2 * D + npar), dtype=torch.float64, device=dev)
    g_params = torch.zeros((B, npar), dtype=torch.float64, device=dev)
    g_y0 = torch.zeros((B, D), dtype=torch.float64, device=dev)
    tiles = (B + 15) // 16
    recf = lib.ionode_grad_record_floats(L, N) if need_w else 0
    partf = lib.ionode_grad_partial_floats(L, N) if need_w else 0
    budget = _bounded_budget(cfg.get("record_budget_bytes"), DEFAULT_RECORD_BUDGET, dev, 0.5)
    acc = torch.zeros(partf, dtype=torch.float64, device=dev) if need_w else None
    main = torch.cuda.current_stream(dev)
    pkd = int(lib.ionode_grad_packet_doubles()) if two_phase else 0
    chunk, n_buf, bounds = plan_backward_chunks(n_iter, tiles, recf, pkd, budget, need_w, two_phase)
    records = [torch.empty(tiles * chunk * 6 * recf, dtype=torch.float32, device=dev) for _ in range(n_buf)] if need_w else [None] * n_buf
    packets = [torch.empty(tiles * chunk * pkd, dtype=torch.float64, device=dev) for _ in range(n_buf)] if two_phase else [None] * n_buf
    side = torch.cuda.Stream(dev) if (need_w and n_buf == 2) else main          # reductions
    pre = torch.cuda.Stream(dev) if (two_phase and n_buf == 2) else main         # phase A
    if pre is not main:
        pre.wait_stream(main)    # g / state / inputs were produced on the caller's stream
    free = [None] * n_buf   # event: the reduce (or, without weight gradients, the walk) that last used this buffer pair has finished
    ready = [None] * n_buf  # event: phase A has filled this buffer pair
    sse_y0 = torch.zeros((B, D), dtype=torch.float64, device=dev) if fused and two_phase else None   # sample-0 term of dL/dy0: written by the last chunk's G_c launch
    # the entry points' buffers by name (capi.SWEEP_BUFFERS): what all seven take, what the launches that run the net add, the adjoint
    shared = dict(prot_v=cfg["prot_v"], prot_t=cfg.get("prot_t"), prot_of_traj=cfg.get("prot_of_traj"), t_eval=cfg["t_eval"], n_accepted=n_acc)
    net = dict(shared, grad_image=image, params=params)
    kind = capi.objective_kind(cfg["objective"]) if fused else None   # the two launches that form the residuals' weights take it
    adjoint = dict(state=state, grad_params=g_params, grad_y0=g_y0)

    def phase_a(k):
        it0, it1 = bounds[k]
        b = k % n_buf
        if free[b] is not None:
            pre.wait_event(free[b])
        if fused:   # G_c of the objective (one wavefront per trajectory and step), then the products without grad_y: same stream, same packets
            capi.objective_launch("ionode_objective_backward_gc", gc_desc, kind, it0, it1, n_iter, pre, grad_sse=g, packets=packets[b],
                                  sse_grad_y0=sse_y0, **shared)
            capi.sweep_launch("ionode_dopri5_backward_recompute_sse", desc, it0, it1, n_iter, pre, records=records[b], packets=packets[b], **net)
        else:
            capi.sweep_launch("ionode_dopri5_backward_recompute", desc, it0, it1, n_iter, pre, grad_y=g, records=records[b],
                              packets=packets[b], **net)
        ev = torch.cuda.Event()
        ev.record(pre)
        ready[b] = ev

    if two_phase:
        phase_a(0)
    for k, (it0, it1) in enumerate(bounds):
        b = k % n_buf
        rec = records[b]
        if two_phase:
            if k + 1 < len(bounds) and n_buf == 2:
                phase_a(k + 1)                      # one chunk ahead, beside this chunk's walk
            main.wait_event(ready[b])
            if fused:
                capi.sweep_launch("ionode_dopri5_backward_sweep_sse", desc, it0, it1, n_iter, main, sse_grad_y0=sse_y0, records=rec,
                                  packets=packets[b], **net, **adjoint)
            else:
                capi.sweep_launch("ionode_dopri5_backward_sweep", desc, it0, it1, n_iter, main, grad_y=g, records=rec, packets=packets[b],
                                  **net, **adjoint)
        else:
            if free[b] is not None:
                main.wait_event(free[b])
            if fused:   # closed-form models: the seed is formed in the kernel; one launch (plan_backward_chunks: nothing to buffer)
                capi.objective_launch("ionode_objective_backward", desc, kind, it0, it1, n_iter, main, params=params, grad_sse=g, **shared, **adjoint)
            else:
                capi.sweep_launch("ionode_dopri5_backward", desc, it0, it1, n_iter, main, grad_y=g, records=rec, **net, **adjoint)
        swept = torch.cuda.Event()
        swept.record(main)
        if need_w:
            n_rec = tiles * (it1 - it0) * 6
            n_slabs = int(os.environ.get("IONODE_GRAD_SLABS", 0)) or int(lib.ionode_grad_reduce_slabs(L, N, n_rec))   # one round of workgroups on this device (env: dev override for A/B runs)
            side.wait_event(swept)
            with torch.cuda.stream(side):
                partials = torch.empty((n_slabs, partf), dtype=torch.float32, device=dev)
                reduce = lib.ionode_grad_reduce_unit if two_phase else lib.ionode_grad_reduce   # unit-seed records: scaled while staged
                rc = reduce(L, N, C.c_void_p(rec.data_ptr()), n_rec, n_slabs, C.c_void_p(partials.data_ptr()), C.c_void_p(side.cuda_stream))
                if rc != 0:
                    raise capi.IonodeError(f"ionode_grad_reduce failed ({rc}): {lib.ionode_grad_last_error().decode()}")
                acc += partials.double().sum(0)
                done = torch.cuda.Event()
                done.record(side)
            free[b] = done
        else:
            free[b] = swept
        if two_phase and n_buf == 1 and k + 1 < len(bounds):
            phase_a(k + 1)                          # single buffer: strictly alternate
    if need_w and side is not main:
        main.wait_stream(side)
    if pre is not main:
        main.wait_stream(pre)
    return acc, g_params, g_y0


def solve(model, weights_flat, params, prot_v, y0, t_eval, *, mlp_layers=0, mlp_width=0, prot_t=None, prot_t0=0.0,
          prot_dt=1.0, prot_of_traj=None, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, max_step=0.0,
          ckpt_cap=None, record_budget_bytes=None, weights_key=None, t_eval_hint="auto", order=None, tile_waves=0,
          ckpt_budget_bytes=None, two_phase=None):
    """Differentiable batched solve.  weights_flat [n] fp32 (reference state-dict order; None for the closed-form HH 2-state
    and 6-state models, whose params are [B, 8] / [B, 12] and y0 [B, 2] / [B, 6]), params [B, 8] fp64, y0 [B, 2]
    fp32 | fp64 (the state dtype) -- device tensors, any of which may require grad; prot_v [P, Np], t_eval [Nt] fp64 device
    tensors.  Returns (y [B, Nt, 2], status [B]): gradients of failed trajectories (status != 0) are zero -- their rows of the
    upstream gradient are ignored (y is NaN-filled there), and dL/dy0, dL/dp rows are zero whether or not the caller masks its loss.
    A failed trajectory never grows the checkpoint buffer; a batch whose successful trajectories need more than
    ckpt_budget_bytes (default 96 GiB) of checkpoints raises IonodeError instead of running out of memory.

    max_step (ms | "auto", extension; 0 = off = the reference's dopri5; "auto" = stable_step_cap(); a RuntimeWarning is issued
    when params requires grad and no cap is set): at an equilibrium dopri5 lets dt grow until h*lambda is far
    outside its stability region (the error estimate of a state AT equilibrium is ~0); the forward solve copes through
    rejections, but the exact derivative of those accepted-but-unstable steps multiplies the adjoint by |R(h*lambda)| >> 1
    per step (measured on the 10 s sine-wave protocol, fp32 state: |dL/dp| ~ 1e36 while dL/dW, whose state `a` is not
    stiff, stays O(100)).  max_step < 3.3 / lambda_max -- 10 ms for the reference's rate constants -- keeps it bounded.

    order (optional permutation of range(B), schedule.lpt_order): launch slot k integrates trajectory order[k] (homogeneous
    tiles, expensive tiles first -- pays from two tiles per compute unit, B > 4096); y and status are then in LAUNCH order
    (row k = trajectory order[k]), and the gradients still arrive at params / y0 in the caller's order (the gather is part of
    the autograd graph)."""
    max_step = _resolve_max_step(model, params, prot_v, v_oob, max_step)
    if model in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        # closed-form models (train-s1.py:161-177, train-d1.py:165-187): gradients w.r.t. the rate parameters and y0; no weights
        if weights_flat is not None:
            raise capi.IonodeError("the closed-form models have no MLP: pass weights_flat=None")
        mlp_layers = mlp_width = 0
    elif model not in (capi.MODEL_NNF, capi.MODEL_NND):
        raise NotImplementedError("unknown model")
    if not (isinstance(y0, torch.Tensor) and y0.is_cuda):
        raise capi.IonodeError("no HIP tensors: the integrator and its backward sweep have no CPU path")
    if order is not None:
        order = torch.as_tensor(order, dtype=torch.int64, device=y0.device)
        B = y0.shape[0]
        if order.shape != (B,) or int(order.min()) < 0 or int(order.max()) >= B or \
                not bool(torch.bincount(order, minlength=B).eq(1).all()):
            raise capi.IonodeError(f"order must be a permutation of range({B})")
        params, y0 = params.index_select(0, order), y0.index_select(0, order)
        pot = prot_of_traj if prot_of_traj is not None else (torch.arange(B, device=y0.device) % prot_v.shape[0]).to(torch.int32)
        prot_of_traj = torch.as_tensor(pot, device=y0.device).index_select(0, order).to(torch.int32).contiguous()
    cfg = dict(model=model, mlp_layers=int(mlp_layers), mlp_width=int(mlp_width), prot_v=prot_v, prot_t=prot_t,
               prot_t0=float(prot_t0), prot_dt=float(prot_dt), prot_of_traj=prot_of_traj, t_eval=t_eval, rtol=float(rtol),
               atol=float(atol), v_oob=float(v_oob), max_steps=int(max_steps), max_total_steps=int(max_total_steps),
               max_step=float(max_step), ckpt_cap=ckpt_cap, record_budget_bytes=record_budget_bytes, weights_key=weights_key, t_eval_hint=t_eval_hint,
               tile_waves=int(tile_waves), ckpt_budget_bytes=ckpt_budget_bytes)
    if two_phase is not None:   # None: the two-phase sweep unless IONODE_GRAD_ONE_PHASE=1; results agree to fp32 rounding (1e-5), not bit for bit: the seed multiplies at the end of the product
        cfg["two_phase"] = bool(two_phase)
    return _Solve.apply(weights_flat, params, y0.contiguous(), cfg)


def allreduce_gradients(tensors, group=None):
    """Sum gradient tensors over the ranks with ONE collective (flattened bucket): RCCL over xGMI under `nccl`.
    For s00 that is 201 801 fp32 = 807 KB -- latency-bound next to a >= 100 ms sweep."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return tensors
    flat = torch.cat([t.reshape(-1).to(torch.float64) for t in tensors])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    out, off = [], 0
    for t in tensors:
        out.append(flat[off:off + t.numel()].reshape(t.shape).to(t.dtype))
        off += t.numel()
    return out


def uniform_grid_hint(t_eval):
    """(t0, dt) of a uniform output grid -- what the fused objective's output cursor needs (ionode_desc.t_eval_dt_hint; the
    kernel verifies it against t_eval) -- or None: capi.dopri5's "auto" rule (capi.uniform_grid: every t_k within dt / 2 of t0 + k dt)."""
    grid = capi.uniform_grid(t_eval)
    return None if grid is None else grid[:2]


def sum_of_squares(model, params, prot_v, y0, t_eval, sse_ref, *, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None,
                   obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0,
                   max_total_steps=0, max_step=0.0, ckpt_cap=None, ckpt_budget_bytes=None, weights_flat=None, mlp_layers=0, mlp_width=0,
                   weights_key=None, record_budget_bytes=None, two_phase=None):
    """Fused sum-of-squares objective with its gradient (PINTS SumOfSquaresError.evaluateS1 over a batch): the closed-form HH
    2-state and 6-state models, and -- with weights_flat -- NN-f and NN-d of every width the backward sweep serves.

    sse[b] = sum_k (i_k - sse_ref[protocol(b)][k])^2, i_k = obs_g * gate(y_k) * (V(t_k) - obs_e), gate = y0 * y1 (or the last
    state with obs_open_state_only), k = 0 .. Nt - 1 (sample 0 is y0): the objective of batched.solve(sse_ref=..., states=False).
    params [B, 8 | 12] fp64, y0 [B, D] fp32 | fp64 (the state dtype), prot_v [P, Np], t_eval [Nt], sse_ref [P, Nt] fp64 -- device
    tensors; params and y0 may require grad.  Returns (sse [B] fp64, status [B] int32), differentiable in params and y0: the exact
    derivative of the discretisation the forward executed, as grad.solve's.  Failed trajectories (status != 0) give sse = inf;
    their upstream values are ignored and their dL/dp, dL/dy0 rows are zero.

    Neither the states nor the current trace nor dL/dy is ever materialised: the forward writes accepted-step checkpoints and
    the per-trajectory sums only, and the backward sweep (ionode_objective_backward, the squares' kind) re-evaluates every output sample from the
    checkpoints and forms dL/dy_k in the kernel.  Memory: the checkpoints (sized, regrown and bounded by ckpt_cap /
    ckpt_budget_bytes as in grad.solve) plus O(B).  The output grid must be uniform (the fused forward's output cursor); for any
    other t_eval use the materialised route, grad.solve followed by the sum of squares in torch.  max_step: as grad.solve.

    NN-f / NN-d: weights_flat [n] fp32 (reference state-dict order, as grad.solve's; it may require grad), mlp_layers, mlp_width,
    weights_key (the weight images' cache key) and record_budget_bytes as in grad.solve; params [B, 8], y0 [B, 2].  The result is
    differentiable in weights_flat, params and y0.  The backward is grad.solve's two-phase sweep with the same chunking, streams and
    reduction; per chunk ionode_objective_backward_gc re-evaluates the steps' output samples from the checkpoints and hands their
    sums to the walk, and the vector-Jacobian products run without an output gradient.  Memory: the checkpoints, the chunk's records
    and packets (record_budget_bytes), O(B) -- nothing of size [B, Nt].  This route is two-phase only: with two_phase=False, or
    IONODE_GRAD_ONE_PHASE=1 in the environment, it raises; the one-phase sweep serves the materialised route (grad.solve)."""
    return _fused_objective("sse", model, params, prot_v, y0, t_eval, sse_ref, prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt,
                            prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol,
                            v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps, max_step=max_step, ckpt_cap=ckpt_cap,
                            ckpt_budget_bytes=ckpt_budget_bytes, weights_flat=weights_flat, mlp_layers=mlp_layers, mlp_width=mlp_width,
                            weights_key=weights_key, record_budget_bytes=record_budget_bytes, two_phase=two_phase)


def sum_of_abs(model, params, prot_v, y0, t_eval, sae_ref, *, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None,
               obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0,
               max_total_steps=0, max_step=0.0, ckpt_cap=None, ckpt_budget_bytes=None, weights_flat=None, mlp_layers=0, mlp_width=0,
               weights_key=None, record_budget_bytes=None, two_phase=None):
    """Fused sum-of-absolute-errors objective with its gradient: the reference's loss torch.mean(torch.abs(pred_yo - data))
    (train-s1.py:329, train-d1.py:305, train-r1.py:275) times the sample count, differentiated through the solve as its
    `odeint_adjoint` import promises -- all four models, as grad.sum_of_squares.

    sae[b] = sum_k |i_k - sae_ref[protocol(b)][k]|, i_k and k as in grad.sum_of_squares: the objective of
    batched.solve(sse_ref=..., objective="sae", states=False), bit for bit.  Arguments, shapes and dtypes are grad.sum_of_squares';
    sae_ref [P, Nt] fp64 holds the reference currents.  Returns (sae [B] fp64, status [B] int32), differentiable in params and y0
    (and in weights_flat for NN-f / NN-d): the exact derivative of the discretisation the forward executed, with
    d|r|/dr = sign(r) and sign(0) = 0, the subgradient torch.abs's backward takes.  Failed trajectories (status != 0) give
    sae = inf; their upstream values are ignored and their dL/dp, dL/dy0 rows are zero.  The mean absolute error of a batch is
    sae.sum() / (B * Nt).

    The launches, the memory (checkpoints plus O(B), and a chunk's records and packets for the NN models: nothing of size [B, Nt]),
    the uniform output grid, max_step and the two-phase-only rule of the NN models are grad.sum_of_squares': one body serves both, the
    kind travels to ionode_objective_backward / ionode_objective_backward_gc, where a sample's adjoint weight is
    dL/dsae[b] sign(r_k) instead of 2 dL/dsse[b] r_k.  For any other t_eval use the materialised route, grad.solve followed by the
    absolute values in torch."""
    return _fused_objective("sae", model, params, prot_v, y0, t_eval, sae_ref, prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt,
                            prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol,
                            v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps, max_step=max_step, ckpt_cap=ckpt_cap,
                            ckpt_budget_bytes=ckpt_budget_bytes, weights_flat=weights_flat, mlp_layers=mlp_layers, mlp_width=mlp_width,
                            weights_key=weights_key, record_budget_bytes=record_budget_bytes, two_phase=two_phase)


def _fused_objective(objective, model, params, prot_v, y0, t_eval, sse_ref, *, prot_t, prot_t0, prot_dt, prot_of_traj, obs_g, obs_e,
                     obs_open_state_only, rtol, atol, v_oob, max_steps, max_total_steps, max_step, ckpt_cap, ckpt_budget_bytes, weights_flat,
                     mlp_layers, mlp_width, weights_key, record_budget_bytes, two_phase):
    """The one body of sum_of_squares ("sse") and sum_of_abs ("sae"): argument checks, cfg, _FusedObjective."""
    who = "grad.sum_of_squares" if objective == "sse" else "grad.sum_of_abs"
    nn = model in (capi.MODEL_NNF, capi.MODEL_NND)
    if not nn and model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        raise NotImplementedError("unknown model")
    if nn and weights_flat is None:
        raise capi.IonodeError(f"{who}: only the closed-form models have no weights; an NN model needs weights_flat, "
                               "mlp_layers and mlp_width")
    if not nn and weights_flat is not None:
        raise capi.IonodeError("the closed-form models have no MLP: pass weights_flat=None")
    if nn and (os.environ.get("IONODE_GRAD_ONE_PHASE", "0") == "1" or (two_phase is not None and not two_phase)):
        raise capi.IonodeError(f"{who}: the fused sweep of the NN models is two-phase only (two_phase=False or "
                               "IONODE_GRAD_ONE_PHASE=1 asks for the one-phase sweep); for that use grad.solve and form the sum in torch")
    max_step = _resolve_max_step(model, params, prot_v, v_oob, max_step, frames=3)
    if not (isinstance(y0, torch.Tensor) and y0.is_cuda):
        raise capi.IonodeError("no HIP tensors: the integrator and its backward sweep have no CPU path")
    D = capi.n_state(model)
    if y0.dim() != 2 or y0.shape[1] != D or params.dim() != 2 or params.shape[0] != y0.shape[0]:
        raise capi.IonodeError(f"params [B, {capi.n_params(model)}] and y0 [B, {D}] expected")
    hint = uniform_grid_hint(t_eval)
    if hint is None:
        raise capi.IonodeError(f"{who} needs a uniform output grid t_eval (the fused objective's output cursor); for "
                               "other grids use the materialised route: grad.solve, then the sum over the current's residuals in torch")
    cfg = dict(model=model, prot_v=prot_v, prot_t=prot_t, prot_t0=float(prot_t0), prot_dt=float(prot_dt), t_eval=t_eval,
               prot_of_traj=None if prot_of_traj is None else torch.as_tensor(prot_of_traj, device=y0.device).to(torch.int32).contiguous(),
               rtol=float(rtol), atol=float(atol), v_oob=float(v_oob), max_steps=int(max_steps), max_total_steps=int(max_total_steps),
               max_step=float(max_step), obs_g=float(obs_g), obs_e=float(obs_e), obs_open_state_only=bool(obs_open_state_only),
               t_eval_hint=hint, sse_ref=sse_ref, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes,
               mlp_layers=int(mlp_layers) if nn else 0, mlp_width=int(mlp_width) if nn else 0, weights_key=weights_key,
               record_budget_bytes=record_budget_bytes, two_phase=True, objective=objective)
    return _FusedObjective.apply(weights_flat, params, y0.contiguous(), cfg)
