"""ctypes binding of libionode.so (include/ionode.h).  torch is used for device memory and streams only.

There is no CPU fallback: if the HIP library is missing or no GPU is visible, the calls raise.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# IONODE_LIB: dev override to A/B kernel builds (tools/ab_build.sh); the default is the in-tree library
LIB_PATH = os.environ.get("IONODE_LIB") or os.path.join(_HERE, "libionode.so")

MODEL_HH2, MODEL_MARKOV6, MODEL_NNF, MODEL_NND = 0, 1, 2, 3
STATUS_OK, STATUS_DT_UNDERFLOW, STATUS_NONFINITE, STATUS_MAX_STEPS = 0, 1, 2, 3
STATUS_TEXT = {
    0: "ok",
    1: "underflow in dt",                 # torchdiffeq's assertion messages
    2: "non-finite values in state `y`",
    3: "max_num_steps exceeded",
}
ABI_VERSION = 10

# the kind of the fused objective (include/ionode.h IONODE_OBJECTIVE_*): what a residual adds to its trajectory's sum
OBJECTIVE_SSE, OBJECTIVE_SAE = 0, 1
OBJECTIVE_KINDS = {"sse": OBJECTIVE_SSE, "sae": OBJECTIVE_SAE}

# the backward sweep's entry points: their buffers in ABI order -- between (d, it_begin, it_end, n_iter) and stream (include/ionode.h;
# tests/test_grad_entry_checks.py compares the names with the header's).  argtypes are generated from it, sweep_launch() calls by it.
SWEEP_BUFFERS = {
    "ionode_dopri5_backward": ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "grad_y", "state",
                               "records", "grad_params", "grad_y0"),
    "ionode_dopri5_backward_sse": ("params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "grad_sse", "state",
                                   "grad_params", "grad_y0"),
    "ionode_dopri5_backward_recompute": ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "grad_y",
                                         "records", "packets"),
    "ionode_dopri5_backward_sweep": ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "grad_y", "state",
                                     "records", "packets", "grad_params", "grad_y0"),
    "ionode_dopri5_backward_sse_gc": ("prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "grad_sse", "packets", "sse_grad_y0"),
    "ionode_dopri5_backward_recompute_sse": ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "records",
                                             "packets"),
    "ionode_dopri5_backward_sweep_sse": ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "sse_grad_y0",
                                         "state", "records", "packets", "grad_params", "grad_y0"),
}

# the fused objective's gradient of either kind (include/ionode.h): the two launches that form the residuals' weights.  Their buffers
# in ABI order -- between (d, objective, it_begin, it_end, n_iter) and stream: those of the squares' entry points, which they are with
# OBJECTIVE_SSE.  objective_launch() calls by these names.
OBJECTIVE_BUFFERS = {
    "ionode_objective_backward": SWEEP_BUFFERS["ionode_dopri5_backward_sse"],
    "ionode_objective_backward_gc": SWEEP_BUFFERS["ionode_dopri5_backward_sse_gc"],
}

# the NN models' tangent sweep (ionode_tangent_sweep_nn): its buffers in ABI order -- between (d, it_begin, it_end, n_iter) and stream
TANGENT_NN_BUFFERS = ("grad_image", "params", "prot_v", "prot_t", "prot_of_traj", "t_eval", "n_accepted", "packets", "state",
                      "di_dp", "jtr", "jtj")


def n_state(model):
    return 6 if model == MODEL_MARKOV6 else 2


def n_params(model):
    return 12 if model == MODEL_MARKOV6 else 8


class IonodeDesc(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("state_f32", C.c_int32), ("n_state", C.c_int32), ("n_out", C.c_int32),
        ("n_traj", C.c_int32), ("n_prot", C.c_int32), ("prot_n", C.c_int32), ("mlp_layers", C.c_int32),
        ("mlp_width", C.c_int32), ("n_params", C.c_int32), ("max_steps", C.c_int64),
        ("prot_t0", C.c_double), ("prot_dt", C.c_double), ("v_oob", C.c_double),
        ("rtol", C.c_double), ("atol", C.c_double), ("obs_g", C.c_double), ("obs_e", C.c_double),
        ("obs_open_state_only", C.c_int32), ("tile_waves", C.c_int32),
        ("step_log", C.c_void_p), ("step_log_cap", C.c_int64),
        ("t_eval_t0_hint", C.c_double), ("t_eval_dt_hint", C.c_double),
        ("max_total_steps", C.c_int64), ("ckpt", C.c_void_p), ("ckpt_cap", C.c_int32), ("t_eval_exact", C.c_int32),
        ("sse_ref", C.c_void_p), ("sse_out", C.c_void_p), ("max_step", C.c_double), ("v_at_outputs", C.c_void_p),
        ("mlp_image_stride", C.c_int64), ("traj_per_image", C.c_int32), ("launch_order", C.c_void_p),
    ]


class IonodeError(RuntimeError):
    pass


# the Levenberg-Marquardt step (include/ionode.h ionode_lm_desc, IONODE_LM_*): descriptor, state layout, stop flags
LM_MAX_FREE, LM_RETRIES, LM_FLOOR_REL, LM_FLOOR_ABS = 12, 8, 2.0 ** -20, 2.0 ** -256
LM_STATE_F, LM_STATE_LAM, LM_STATE_NU, LM_STATE_PRED, LM_STATE_U = 0, 1, 2, 3, 4
LM_RUNNING, LM_GTOL, LM_XTOL, LM_FTOL, LM_STALLED, LM_MAXITER, LM_NONFINITE = range(7)
LM_FLAG_TEXT = {0: "running", 1: "gradient below gtol", 2: "step below xtol", 3: "reduction below ftol", 4: "stalled (damping above lam_max)",
                5: "iteration cap", 6: "non-finite start or derivative"}


class IonodeLmDesc(C.Structure):
    _fields_ = [
        ("n_cand", C.c_int32), ("n_active", C.c_int32), ("n_prot", C.c_int32), ("n_params", C.c_int32),
        ("n_free", C.c_int32), ("log_parameters", C.c_int32), ("max_iter", C.c_int32), ("reserved", C.c_int32),
        ("free_idx", C.c_int32 * LM_MAX_FREE), ("base", C.c_double * LM_MAX_FREE),
        ("lo", C.c_double * LM_MAX_FREE), ("hi", C.c_double * LM_MAX_FREE),
        ("gtol", C.c_double), ("xtol", C.c_double), ("ftol", C.c_double), ("rho_accept", C.c_double), ("lam_max", C.c_double),
    ]


def lm_state_doubles(nf):
    """fp64 words of one candidate's Levenberg-Marquardt state: f, lam, nu, pred, then u, x, g, ut, xt, delta [nf] and H [nf][nf]."""
    return LM_STATE_U + 6 * nf + nf * nf


def lm_state_views(state, nf):
    """Named views of a state array [C, lm_state_doubles(nf)] (numpy or torch): f, lam, nu, pred [C]; u, x, g, ut, xt, delta [C, nf];
    H [C, nf, nf]."""
    o = LM_STATE_U
    v = {"f": state[:, LM_STATE_F], "lam": state[:, LM_STATE_LAM], "nu": state[:, LM_STATE_NU], "pred": state[:, LM_STATE_PRED]}
    for k, name in enumerate(("u", "x", "g", "ut", "xt", "delta")):
        v[name] = state[:, o + k * nf:o + (k + 1) * nf]
    v["H"] = state[:, o + 6 * nf:o + 6 * nf + nf * nf].reshape(state.shape[0], nf, nf)
    return v


# the CMA-ES step (include/ionode.h ionode_cmaes_desc, IONODE_CMAES_*): descriptor, state layout, stop flags
CMAES_MAX_LAMBDA, CMAES_RESAMPLES, CMAES_JACOBI_SWEEPS, CMAES_CONDITION_LIMIT = 64, 8, 30, 1e7
(CMAES_STATE_SIGMA, CMAES_STATE_SIGMA_OLD, CMAES_STATE_BEST_F, CMAES_STATE_F_SIG, CMAES_STATE_UNCHANGED, CMAES_STATE_HSIG,
 CMAES_STATE_NFINITE, CMAES_STATE_FLAG, CMAES_STATE_ROT_C, CMAES_STATE_ROT_S, CMAES_STATE_NROT, CMAES_STATE_COND, CMAES_STATE_M) = range(13)
CMAES_RUNNING, CMAES_MAXITER, CMAES_UNCHANGED, CMAES_TOLX, CMAES_CONDITION, CMAES_NONFINITE = range(6)
CMAES_FLAG_TEXT = {0: "running", 1: "generation cap", 2: "best value unchanged (PINTS' rule)", 3: "step size below tolx",
                   4: "condition of C above the limit", 5: "fewer than mu finite values, or a non-finite state"}


class IonodeCmaesDesc(C.Structure):
    _fields_ = [
        ("n_run", C.c_int32), ("n_active", C.c_int32), ("lambda", C.c_int32), ("n_prot", C.c_int32), ("n_params", C.c_int32),
        ("n_free", C.c_int32), ("log_parameters", C.c_int32), ("max_iter", C.c_int32), ("unchanged_iters", C.c_int32),
        ("run_base", C.c_int32), ("unchanged_threshold", C.c_double), ("tolx", C.c_double), ("seed", C.c_int64),
        ("free_idx", C.c_int32 * LM_MAX_FREE), ("base", C.c_double * LM_MAX_FREE),
        ("lo", C.c_double * LM_MAX_FREE), ("hi", C.c_double * LM_MAX_FREE),
    ]


def cmaes_default_lambda(n):
    """Hansen's default population size 4 + floor(3 ln n)."""
    return 4 + int(np.floor(3.0 * np.log(n)))


def cmaes_state_doubles(n, lam):
    """fp64 words of one run's CMA-ES state: the scalars, 8 vectors [n], 3 matrices [n][n], f and w [lam], the points u and x [lam][n]."""
    return CMAES_STATE_M + 8 * n + 3 * n * n + 2 * lam + 2 * lam * n


def cmaes_state_views(state, n, lam):
    """Named views of a state array [K, cmaes_state_doubles(n, lam)] (numpy or torch): sigma, sigma_old, best_f, f_sig, unchanged,
    hsig, nfinite, flag, cond [K]; m, m_old, pc, ps, D, best_x, yw, zw [K, n]; C, B, A [K, n, n]; f, w [K, lam]; pop, pop_x [K, lam, n]."""
    K = state.shape[0]
    v = {name: state[:, k] for name, k in (("sigma", CMAES_STATE_SIGMA), ("sigma_old", CMAES_STATE_SIGMA_OLD), ("best_f", CMAES_STATE_BEST_F),
                                           ("f_sig", CMAES_STATE_F_SIG), ("unchanged", CMAES_STATE_UNCHANGED), ("hsig", CMAES_STATE_HSIG),
                                           ("nfinite", CMAES_STATE_NFINITE), ("flag", CMAES_STATE_FLAG), ("cond", CMAES_STATE_COND))}
    o = CMAES_STATE_M
    for name in ("m", "m_old", "pc", "ps", "D", "best_x", "yw", "zw"):
        v[name] = state[:, o:o + n]
        o += n
    for name in ("C", "B", "A"):
        v[name] = state[:, o:o + n * n].reshape(K, n, n)
        o += n * n
    for name in ("f", "w"):
        v[name] = state[:, o:o + lam]
        o += lam
    for name in ("pop", "pop_x"):
        v[name] = state[:, o:o + lam * n].reshape(K, lam, n)
        o += lam * n
    return v


# the adaptive-Metropolis step (include/ionode.h ionode_mcmc_desc, IONODE_MCMC_*): descriptor, state layout, stop flags
MCMC_MAX_DIM = 13
MCMC_STATE_LP, MCMC_STATE_LOG_LAMBDA, MCMC_STATE_OUTSIDE, MCMC_STATE_ALPHA, MCMC_STATE_U = range(5)
MCMC_RUNNING, MCMC_MAXITER, MCMC_DEGENERATE, MCMC_NONFINITE = range(4)
MCMC_FLAG_TEXT = {0: "running", 1: "iteration cap", 2: "proposal covariance not positive definite, or a non-finite adaptation state",
                  3: "start outside the box, or its log-posterior not finite"}


class IonodeMcmcDesc(C.Structure):
    _fields_ = [
        ("n_chain", C.c_int32), ("n_active", C.c_int32), ("n_prot", C.c_int32), ("n_params", C.c_int32), ("n_free", C.c_int32),
        ("log_parameters", C.c_int32), ("sample_sigma", C.c_int32), ("max_iter", C.c_int32), ("adapt_start", C.c_int32),
        ("thin", C.c_int32), ("sample_cap", C.c_int32), ("chain_base", C.c_int32), ("seed", C.c_int64),
        ("n_samples", C.c_double), ("sigma", C.c_double), ("sigma_lo", C.c_double), ("sigma_hi", C.c_double),
        ("eta", C.c_double), ("target_accept", C.c_double), ("epsilon", C.c_double),
        ("free_idx", C.c_int32 * LM_MAX_FREE), ("base", C.c_double * LM_MAX_FREE),
        ("lo", C.c_double * LM_MAX_FREE), ("hi", C.c_double * LM_MAX_FREE),
    ]


def mcmc_state_doubles(n):
    """fp64 words of one chain's adaptive-Metropolis state: lp, log_lambda, the outside word, alpha, then u, ut, x, xt, mu [n] and
    C, L [n][n]; n = the free parameters plus one if sigma is sampled."""
    return MCMC_STATE_U + 5 * n + 2 * n * n


def mcmc_state_views(state, nf, sample_sigma):
    """Named views of a state array [K, mcmc_state_doubles(n)] (numpy or torch), n = nf + (1 if sample_sigma else 0): lp, log_lambda,
    outside, alpha [K]; u, ut, x, xt, mu [K, n]; C, L [K, n, n]."""
    n = nf + (1 if sample_sigma else 0)
    K = state.shape[0]
    v = {"lp": state[:, MCMC_STATE_LP], "log_lambda": state[:, MCMC_STATE_LOG_LAMBDA], "outside": state[:, MCMC_STATE_OUTSIDE],
         "alpha": state[:, MCMC_STATE_ALPHA]}
    o = MCMC_STATE_U
    for name in ("u", "ut", "x", "xt", "mu"):
        v[name] = state[:, o:o + n]
        o += n
    for name in ("C", "L"):
        v[name] = state[:, o:o + n * n].reshape(K, n, n)
        o += n * n
    return v


# the manifold-MALA step (include/ionode.h ionode_mala_desc, IONODE_MALA_*): descriptor, state layout, stop flags
MALA_STATE_LP, MALA_STATE_LOG_EPS, MALA_STATE_OUTSIDE, MALA_STATE_ALPHA, MALA_STATE_LD, MALA_STATE_LQF, MALA_STATE_U = range(7)
MALA_RUNNING, MALA_MAXITER, MALA_DEGENERATE, MALA_NONFINITE = range(4)
MALA_FLAG_TEXT = {0: "running", 1: "iteration cap", 2: "the start's metric (J^T J / sigma^2 with its ridge) is not positive definite",
                  3: "start outside the box, or its log-posterior not finite"}


class IonodeMalaDesc(C.Structure):
    _fields_ = [
        ("n_chain", C.c_int32), ("n_active", C.c_int32), ("n_prot", C.c_int32), ("n_params", C.c_int32), ("n_free", C.c_int32),
        ("log_parameters", C.c_int32), ("sample_sigma", C.c_int32), ("max_iter", C.c_int32), ("thin", C.c_int32),
        ("sample_cap", C.c_int32), ("chain_base", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_int64),
        ("n_samples", C.c_double), ("sigma", C.c_double), ("sigma_lo", C.c_double), ("sigma_hi", C.c_double),
        ("eta", C.c_double), ("target_accept", C.c_double), ("ridge", C.c_double),
        ("free_idx", C.c_int32 * LM_MAX_FREE), ("base", C.c_double * LM_MAX_FREE),
        ("lo", C.c_double * LM_MAX_FREE), ("hi", C.c_double * LM_MAX_FREE),
    ]


def mala_state_doubles(n):
    """fp64 words of one chain's manifold-MALA state: lp, log_eps, the outside word, alpha, ld, lq_f, then u, ut, x, xt, grad [n] and
    L [n][n]; n = the free parameters plus one if sigma is sampled."""
    return MALA_STATE_U + 5 * n + n * n


def mala_state_views(state, nf, sample_sigma):
    """Named views of a state array [K, mala_state_doubles(n)] (numpy or torch), n = nf + (1 if sample_sigma else 0): lp, log_eps,
    outside, alpha, ld, lqf [K]; u, ut, x, xt, grad [K, n]; L [K, n, n]."""
    n = nf + (1 if sample_sigma else 0)
    v = {"lp": state[:, MALA_STATE_LP], "log_eps": state[:, MALA_STATE_LOG_EPS], "outside": state[:, MALA_STATE_OUTSIDE],
         "alpha": state[:, MALA_STATE_ALPHA], "ld": state[:, MALA_STATE_LD], "lqf": state[:, MALA_STATE_LQF]}
    o = MALA_STATE_U
    for name in ("u", "ut", "x", "xt", "grad"):
        v[name] = state[:, o:o + n]
        o += n
    v["L"] = state[:, o:o + n * n].reshape(state.shape[0], n, n)
    return v


# the affine-invariant ensemble step (include/ionode.h ionode_ensemble_desc, IONODE_ENSEMBLE_*): descriptor, state layout, flags, moves
ENSEMBLE_MAX_WALKERS = 4096
ENSEMBLE_STATE_LP, ENSEMBLE_STATE_LQ, ENSEMBLE_STATE_OUTSIDE, ENSEMBLE_STATE_U = range(4)
ENSEMBLE_RUNNING, ENSEMBLE_MAXITER, ENSEMBLE_NONFINITE = range(3)
ENSEMBLE_STRETCH, ENSEMBLE_DE = 0, 1
ENSEMBLE_MOVES = {"stretch": ENSEMBLE_STRETCH, "de": ENSEMBLE_DE}
ENSEMBLE_FLAG_TEXT = {0: "running", 1: "iteration cap", 2: "a start outside the box, or its log-posterior not finite"}
ENSEMBLE_ROLE_ASK, ENSEMBLE_ROLE_ACCEPT, ENSEMBLE_ROLE_JITTER, ENSEMBLE_ROLE_SPREAD = range(4)   # the generator's fourth counter word / 65536


class IonodeEnsembleDesc(C.Structure):
    _fields_ = [
        ("n_ens", C.c_int32), ("n_walkers", C.c_int32), ("n_prot", C.c_int32), ("n_params", C.c_int32), ("n_free", C.c_int32),
        ("log_parameters", C.c_int32), ("sample_sigma", C.c_int32), ("max_iter", C.c_int32), ("thin", C.c_int32),
        ("sample_cap", C.c_int32), ("ensemble_base", C.c_int32), ("move", C.c_int32), ("seed", C.c_int64),
        ("n_samples", C.c_double), ("sigma", C.c_double), ("sigma_lo", C.c_double), ("sigma_hi", C.c_double),
        ("a", C.c_double), ("gamma", C.c_double), ("jitter", C.c_double),
        ("free_idx", C.c_int32 * LM_MAX_FREE), ("base", C.c_double * LM_MAX_FREE),
        ("lo", C.c_double * LM_MAX_FREE), ("hi", C.c_double * LM_MAX_FREE),
    ]


def ensemble_state_doubles(n):
    """fp64 words of one walker's state: lp, lq, the outside word, then u, ut, x, xt [n]; n = the free parameters plus one if sigma
    is sampled."""
    return ENSEMBLE_STATE_U + 4 * n


def ensemble_state_views(state, nf, sample_sigma):
    """Named views of a state array [E, W, ensemble_state_doubles(n)] (numpy or torch), n = nf + (1 if sample_sigma else 0): lp, lq,
    outside [E, W]; u, ut, x, xt [E, W, n]."""
    n = nf + (1 if sample_sigma else 0)
    v = {"lp": state[..., ENSEMBLE_STATE_LP], "lq": state[..., ENSEMBLE_STATE_LQ], "outside": state[..., ENSEMBLE_STATE_OUTSIDE]}
    o = ENSEMBLE_STATE_U
    for name in ("u", "ut", "x", "xt"):
        v[name] = state[..., o:o + n]
        o += n
    return v


# the posterior predictive bands (include/ionode.h ionode_predictive_desc, IONODE_PREDICTIVE_*)
PREDICTIVE_MAX_DRAWS = 16384
PREDICTIVE_MAX_Q = 16
PREDICTIVE_TAG = 0x70720000


class IonodePredictiveDesc(C.Structure):
    _fields_ = [
        ("n_prot", C.c_int32), ("n_out", C.c_int32), ("n_draw", C.c_int32), ("s_cap", C.c_int32), ("draw_base", C.c_int32),
        ("draw_offset", C.c_int32), ("noise", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_int64), ("sigma", C.c_double),
    ]


# Every symbol of include/ionode.h: name -> (restype, argtypes); lib() applies the table, EXPORTS is its keys.
_D, _P, _I32, _I64, _F32 = C.POINTER(IonodeDesc), C.c_void_p, C.c_int32, C.c_int64, C.c_float
_SOLVE = [_D] + [_P] * 12   # ionode_dopri5: d, mlp_packed .. stats, stream -- the solve family's common prefix
_REDUCE = [_I32, _I32, _P, _I64, _I32, _P, _P]
PROTOTYPES = {
    "ionode_abi_version": (_I32, []),
    "ionode_last_error": (C.c_char_p, []),
    "ionode_mlp_packed_floats": (C.c_size_t, [_I32, _I32]),
    "ionode_mlp_pack": (C.c_int, [_P, _I32, _I32, _P]),
    "ionode_launch_geometry": (C.c_int, [_D, C.POINTER(_I32 * 4)]),
    "ionode_kernel_name": (C.c_char_p, [_D]),
    "ionode_last_kernel_name": (C.c_char_p, []),
    "ionode_lane_wise_from": (_I32, [_I32, _I32]),
    "ionode_dopri5": (C.c_int, _SOLVE),
    "ionode_dopri5_deferred": (C.c_int, _SOLVE + [_P, _I64]),                    # + workspace, workspace_bytes
    "ionode_dopri5_composed": (C.c_int, _SOLVE + [_P, _I64, _I32]),              # + cost_source
    "ionode_dopri5_objective": (C.c_int, _SOLVE + [_P, _I64, _I32, _I32]),       # + objective
    "ionode_protocol_at_outputs": (C.c_int, [_D] + [_P] * 5),
    "ionode_dense_defer_plan": (C.c_int, [_D, _I32, C.POINTER(_I64 * 2)]),
    "ionode_dense_tail_plan": (C.c_int, [_D, _I32, C.POINTER(_I64 * 2)]),
    "ionode_compose_tail_plan": (C.c_int, [_D, _I32, _I32, C.POINTER(_I64 * 2)]),
    "ionode_compose_plan": (C.c_int, [_D, _I32, C.POINTER(_I32 * 2)]),
    "ionode_compose_order": (C.c_int, [_P, _I32, _I64, _I32, _P, _P]),
    "ionode_compose_order_host": (C.c_int, [_P, _I32, _P]),
    "ionode_grad_last_error": (C.c_char_p, []),
    "ionode_grad_image_floats": (C.c_size_t, [_I32, _I32]),
    "ionode_grad_record_floats": (C.c_size_t, [_I32, _I32]),
    "ionode_grad_partial_floats": (C.c_size_t, [_I32, _I32]),
    "ionode_grad_pack": (C.c_int, [_P, _I32, _I32, _P]),
    "ionode_grad_packet_doubles": (C.c_size_t, []),
    **{name: (C.c_int, [_D] + [_I32] * 3 + [_P] * (len(buffers) + 1)) for name, buffers in SWEEP_BUFFERS.items()},
    **{name: (C.c_int, [_D] + [_I32] * 4 + [_P] * (len(buffers) + 1)) for name, buffers in OBJECTIVE_BUFFERS.items()},
    "ionode_tangent_sweep": (C.c_int, [_D] + [_P] * 10),   # params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, di_dp, jtr, jtj, stream
    "ionode_tangent_nn_state_doubles": (C.c_size_t, []),
    "ionode_tangent_sweep_nn": (C.c_int, [_D] + [_I32] * 3 + [_P] * (len(TANGENT_NN_BUFFERS) + 1)),
    # d, active, sse, jtr, jtj, status, state, flag, iters, trial (, stream)
    "ionode_lm_step":(C.c_int, [C.POINTER(IonodeLmDesc)] + [_P] * 10),
    "ionode_lm_step_host": (C.c_int, [C.POINTER(IonodeLmDesc)] + [_P] * 9),
    # d, active, value, status, state, flag, iters, trial (, stream)
    "ionode_cmaes_step": (C.c_int, [C.POINTER(IonodeCmaesDesc)] + [_P] * 8),
    "ionode_cmaes_step_host": (C.c_int, [C.POINTER(IonodeCmaesDesc)] + [_P] * 7),
    "ionode_cmaes_draw_host": (None, [_I64] + [_I32] * 5 + [C.POINTER(C.c_uint32 * 4), C.POINTER(C.c_double * 2)]),
    "ionode_cmaes_log_host": (C.c_double, [C.c_double]),
    # d, active, value, status, state, flag, iters, trial, samples (, stream)
    "ionode_mcmc_step": (C.c_int, [C.POINTER(IonodeMcmcDesc)] + [_P] * 9),
    "ionode_mcmc_step_host": (C.c_int, [C.POINTER(IonodeMcmcDesc)] + [_P] * 8),
    # d, active, sse, jtr, jtj, status, state, flag, iters, trial, samples (, stream)
    "ionode_mala_step": (C.c_int, [C.POINTER(IonodeMalaDesc)] + [_P] * 11),
    "ionode_mala_step_host": (C.c_int, [C.POINTER(IonodeMalaDesc)] + [_P] * 10),
    # d, value, status, state, flag, iters, accepted, trial, samples (, stream)
    "ionode_ensemble_step": (C.c_int, [C.POINTER(IonodeEnsembleDesc)] + [_P] * 9),
    "ionode_ensemble_step_host": (C.c_int, [C.POINTER(IonodeEnsembleDesc)] + [_P] * 8),
    # n_run, n_active, lambda, n_params, active, seg_of_run, seg_off, t_rel, a, trial, value, status (, stream)
    "ionode_multi_exp_objective": (C.c_int, [_I32] * 4 + [_P] * 9),
    "ionode_multi_exp_objective_host": (C.c_int, [_I32] * 4 + [_P] * 8),
    # n_seg, n_params, x, full_off, t_full, a_fit, dadt, d2adt2 (, stream)
    "ionode_multi_exp_eval": (C.c_int, [_I32] * 2 + [_P] * 7),
    "ionode_multi_exp_eval_host": (C.c_int, [_I32] * 2 + [_P] * 6),
    # n, mlp_layers, mlp_width, then: acc, padmap, grad, norm_partials (, stream)
    "ionode_train_norm_partials": (_I32, [_I32]),
    "ionode_train_grad_norm": (C.c_int, [_I32] * 3 + [_P] * 5),
    "ionode_train_grad_norm_host": (C.c_int, [_I32] * 3 + [_P] * 4),
    # ... grad, norm_partials, loss, state_in, state_out, weights, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, max_norm (, stream)
    "ionode_train_apply": (C.c_int, [_I32] * 3 + [_P] * 8 + [_F32, C.c_double, C.c_double, _F32, C.c_double, _P]),
    "ionode_train_apply_host": (C.c_int, [_I32] * 3 + [_P] * 8 + [_F32, C.c_double, C.c_double, _F32, C.c_double]),
    # ... forward_map, grad_map, weights, forward_image, grad_image (, stream)
    "ionode_train_refresh": (C.c_int, [_I32] * 3 + [_P] * 6),
    "ionode_train_refresh_host": (C.c_int, [_I32] * 3 + [_P] * 5),
    "ionode_predictive_plan": (C.c_int, [_I32] * 3 + [_I64, C.POINTER(_I64 * 3)]),
    # d, trace, status, sigma, mean, m2, min, max, count, cols (, stream)
    "ionode_predictive_accumulate": (C.c_int, [C.POINTER(IonodePredictiveDesc)] + [_P] * 10),
    "ionode_predictive_accumulate_host": (C.c_int, [C.POINTER(IonodePredictiveDesc)] + [_P] * 9),
    # n_prot, n_out, s_cap, n_q, then: q (host), count, cols, quant (, stream)
    "ionode_predictive_quantiles": (C.c_int, [_I32] * 4 + [_P] * 5),
    "ionode_predictive_quantiles_host": (C.c_int, [_I32] * 4 + [_P] * 4),
    "ionode_grad_reduce": (C.c_int, _REDUCE),
    "ionode_grad_reduce_unit": (C.c_int, _REDUCE),
    "ionode_grad_reduce_slabs": (_I32, [_I32, _I32, _I64]),
    "ionode_regress_step": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _I32, _F32, _P, _P, _I32, _P]),
    "ionode_regress_plan": (C.c_int, [_I32, _I32, C.POINTER(_I32 * 3)]),
    "ionode_adam_step": (C.c_int, [_I32] * 4 + [_P] * 5 + [_F32] * 4 + [_I32, _P, _I32, _P]),
    "ionode_image_refresh": (C.c_int, [_I32, _I32, _P, _P, _P, _P]),
}
EXPORTS = tuple(PROTOTYPES)


def ckpt_record_doubles(D):
    """fp64 words of one accepted-step checkpoint record [t0, dt, oi, nout, y[D], k1..k7[D]] (csrc/ionode_grad_step.hpp CkptRecord)."""
    return 4 + 8 * D


def build(force=False, jobs=8):
    """Compile libionode.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "-s", "clean"])
    subprocess.check_call(["make", "-C", csrc, "-s", f"-j{jobs}"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IonodeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback for the integrator)")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if L.ionode_abi_version() != ABI_VERSION:
            raise IonodeError("libionode.so ABI version mismatch; rebuild")
        _lib = L
    return _lib


def last_error():
    return lib().ionode_last_error().decode()


def state_dict_floats(w, L, N):
    """Floats of the reference's flat state dict of an (L, N) net -- W0[N][2], b0[N], L x (W[N][N], b[N]), wl[N], bl -- after checking
    that the flat array `w` has that many."""
    expect = 2 * N + N + L * (N * N + N) + N + 1
    if w.size != expect:
        raise IonodeError(f"state dict has {w.size} floats, (L={L}, N={N}) needs {expect}")
    return expect


def mlp_pack(state_dict_flat, mlp_layers, mlp_width):
    """Flat fp32 state dict (numpy, reference order) -> packed fp32 image (numpy) for upload."""
    w = np.ascontiguousarray(np.asarray(state_dict_flat, dtype=np.float32).reshape(-1))
    N, L = int(mlp_width), int(mlp_layers)
    state_dict_floats(w, L, N)
    out = np.empty(lib().ionode_mlp_packed_floats(L, N), dtype=np.float32)
    rc = lib().ionode_mlp_pack(w.ctypes.data, L, N, out.ctypes.data)
    if rc != 0:
        raise IonodeError(last_error())
    return out


def library_digest():
    """sha256 of the libionode.so this process uses (bench.py / tools/pmc_summary.py: ties counter evidence to a build)."""
    import hashlib
    h = hashlib.sha256()
    with open(LIB_PATH, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()


def make_desc(**kw):
    d = IonodeDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def launch_geometry(desc):
    out = (C.c_int32 * 4)()
    rc = lib().ionode_launch_geometry(C.byref(desc), C.byref(out))
    if rc != 0:
        raise IonodeError(last_error())
    return {"grid": out[0], "block": out[1], "lds_bytes": out[2], "tile_waves": out[3]}


def regress_plan(mlp_layers, mlp_width):
    """Plan of the regression step at (L, N), pure host code (ionode_regress_plan): which kernel serves it, its workgroups per compute
    unit and its LDS.  Raises IonodeError with the library's message for a shape nothing serves."""
    out = (C.c_int32 * 3)()
    if lib().ionode_regress_plan(int(mlp_layers), int(mlp_width), C.byref(out)) != 0:
        raise IonodeError(lib().ionode_grad_last_error().decode())
    return {"generic": bool(out[0]), "wg_per_cu": out[1], "lds_bytes": out[2]}


def predictive_plan(n_prot, n_out, s_cap, budget_bytes=0):
    """Plan of the predictive bands' quantile pass, pure host code (ionode_predictive_plan): the LDS bytes of the kernel that sorts a
    column of s_cap draws, the sort length's logarithm and the bytes of the column store [n_prot, n_out, s_cap].  Raises IonodeError
    with the library's message for s_cap above PREDICTIVE_MAX_DRAWS and for a store above budget_bytes (0: no budget)."""
    out = (C.c_int64 * 3)()
    if lib().ionode_predictive_plan(int(n_prot), int(n_out), int(s_cap), int(budget_bytes), C.byref(out)) != 0:
        raise IonodeError(lib().ionode_grad_last_error().decode())
    return {"lds_bytes": int(out[0]), "cols_bytes": int(out[1]), "sort_log2": int(out[2])}


def dense_defer_plan(desc, want_current):
    """Deferred dense output of the lean N = 200 16-tile (ionode_dense_defer_plan, pure host code): records per trajectory and
    workspace bytes ionode_dopri5_deferred wants for `desc`; capacity 0: nothing is deferred."""
    out = (C.c_int64 * 2)()
    if lib().ionode_dense_defer_plan(C.byref(desc), int(bool(want_current)), C.byref(out)) != 0:
        raise IonodeError(last_error())
    return {"capacity": int(out[0]), "workspace_bytes": int(out[1])}


def dense_tail_plan(desc, want_current):
    """The solve kernel's tail (ionode_dense_tail_plan, pure host code): how many tiles, in the order they end, expand their own records
    inside the solve kernel, and the records a trajectory may fill (capacity - 1 with the tail on: the last slot holds the counter)."""
    out = (C.c_int64 * 2)()
    if lib().ionode_dense_tail_plan(C.byref(desc), int(bool(want_current)), C.byref(out)) != 0:
        raise IonodeError(last_error())
    return {"tail_rank": int(out[0]), "usable_capacity": int(out[1])}


COST_SOURCE = {None: 0, "pilot": 1, "hint": 2, "explicit": 2}   # ionode_dopri5_composed's cost_source of dopri5()["composed"]
COMPOSE_SOURCES = {0: "off", 1: "pilot", 2: "hint", 3: "auto"}
# the pilot of the tile composition: HH 2-state on the same protocols (schedule.pilot_cost's model).  A loose tolerance ranks the
# trajectories as well as the solve's own (composed maximum 313.7 ms at 1e-4 / 1e-6 against 313.3 at 1e-7 / 1e-9) at 40 % of the attempts
PILOT_RTOL, PILOT_ATOL = 1e-4, 1e-6
PILOT_MAX_ATTEMPTS = 100000   # runaway bound of a pilot trajectory (the headline's take about 1100): it then simply ranks heaviest


def compose_plan(desc, want_current):
    """Shrink-aware tile composition (ionode_compose_plan): does `desc` qualify, and which cost source IONODE_COMPOSE allows."""
    out = (C.c_int32 * 2)()
    if lib().ionode_compose_plan(C.byref(desc), int(bool(want_current)), C.byref(out)) != 0:
        raise IonodeError(last_error())
    return {"compose": bool(out[0]), "source": COMPOSE_SOURCES[int(out[1])]}


def compose_tail_plan(desc, want_current, composed):
    """dense_tail_plan for a launch composed from `composed` (dopri5()["composed"]: None, "pilot", "hint", "explicit")."""
    out = (C.c_int64 * 2)()
    if lib().ionode_compose_tail_plan(C.byref(desc), int(bool(want_current)), COST_SOURCE[composed], C.byref(out)) != 0:
        raise IonodeError(last_error())
    return {"tail_rank": int(out[0]), "usable_capacity": int(out[1])}


def compose_order_host(cost):
    """The composition rule on the host (ionode_compose_order_host): cost [B] -> int32 launch order [B], numpy."""
    c = np.ascontiguousarray(np.asarray(cost, dtype=np.float64).reshape(-1))
    order = np.empty(c.size, dtype=np.int32)
    if lib().ionode_compose_order_host(c.ctypes.data, int(c.size), order.ctypes.data) != 0:
        raise IonodeError(last_error())
    return order


def compose_order(cost, stream=None):
    """The composition rule on the device (ionode_compose_order), asynchronous on the current stream: cost is a 1-D fp64 or int64
    device tensor of any stride (a column of a stats tensor is read in place) -> int32 launch order [B]."""
    if not isinstance(cost, torch.Tensor) or not cost.is_cuda or cost.dim() != 1 or cost.dtype not in (torch.float64, torch.int64) \
            or cost.shape[0] < 1 or (cost.shape[0] > 1 and cost.stride(0) < 1):
        raise IonodeError("cost: expected a 1-D float64 or int64 CUDA/HIP tensor with a positive stride")
    B = int(cost.shape[0])
    order = torch.empty((B,), dtype=torch.int32, device=cost.device)
    s = stream if stream is not None else torch.cuda.current_stream(cost.device).cuda_stream
    rc = lib().ionode_compose_order(C.c_void_p(cost.data_ptr()), int(cost.dtype == torch.int64), max(1, int(cost.stride(0))), B,
                                    C.c_void_p(order.data_ptr()), C.c_void_p(s))
    if rc != 0:
        raise IonodeError(f"ionode_compose_order failed ({rc}): {last_error()}")
    return order


def kernel_name(desc):
    return lib().ionode_kernel_name(C.byref(desc)).decode()


def _dev_ptr(t, dtype, name, shape=None):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise IonodeError(f"{name}: expected a CUDA/HIP tensor (the integrator has no CPU path)")
    if t.dtype != dtype or not t.is_contiguous():
        raise IonodeError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise IonodeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr())


def objective_kind(objective):
    """"sse" | "sae" -> IONODE_OBJECTIVE_SSE | IONODE_OBJECTIVE_SAE; anything else raises IonodeError."""
    kind = OBJECTIVE_KINDS.get(objective) if isinstance(objective, str) else None
    if kind is None:
        raise IonodeError(f"objective: 'sse' (sum of squared residuals) or 'sae' (sum of absolute residuals), got {objective!r}")
    return kind


_order_cache = {}


def _protocol_major(prot_of_traj):
    """Stable argsort of the protocol indices (int32, device), cached per tensor version: the launch order in which the
    trajectories of one protocol are adjacent.  Already-sorted inputs return None (index order)."""
    key = (prot_of_traj.data_ptr(), prot_of_traj._version, int(prot_of_traj.shape[0]), str(prot_of_traj.device))
    hit = _order_cache.get(key)
    if hit is None:
        p = prot_of_traj.to(torch.int64)
        if bool((p[1:] >= p[:-1]).all()):
            hit = (None,)
        else:
            order = torch.argsort(p, stable=True)
            # XCD-aware: workgroups go round-robin over the 8 XCDs (each with its own 4 MB L2), so consecutive wavefronts of the
            # protocol-sorted list would spread every protocol over all eight L2s.  Deal the sorted list out in eight contiguous
            # parts instead -- wavefront i takes wavefront i // 8 of part i % 8 -- and an XCD sees one eighth of the protocols.
            n = int(order.shape[0])
            if n % (64 * 8) == 0:
                order = order.view(8, n // (64 * 8), 64).transpose(0, 1).reshape(-1)
            hit = (order.to(torch.int32).contiguous(),)
        if len(_order_cache) > 8:
            _order_cache.clear()
        _order_cache[key] = hit
    return hit[0]


# ---- the steps of dopri5(), in the order it takes them ----

def _grid_hint(desc, t_eval, t_eval_hint, t_eval_exact):
    """Output-grid hint (t0, dt) into `desc`: a guess the kernel verifies against t_eval; "auto" derives it from the end points
    (one tiny device->host read), None disables it (cooperative scan)."""
    if isinstance(t_eval_hint, str) and t_eval_hint == "auto":
        t_eval_hint = uniform_grid(t_eval)   # pass t_eval_hint=(t0, dt) to avoid its device->host read
        if t_eval_hint is not None and t_eval_exact is None:
            t_eval_exact = t_eval_hint[2] == 0.0
    if t_eval_hint is not None and t_eval_hint[1] > 0:
        desc.t_eval_t0_hint, desc.t_eval_dt_hint = float(t_eval_hint[0]), float(t_eval_hint[1])
        if t_eval_exact is None:
            # exactness is a CLAIM the kernel relies on: verify it here (one tiny device->host read) unless the caller did
            k = torch.arange(desc.n_out, dtype=torch.float64, device=t_eval.device)
            t_eval_exact = bool(torch.equal(t_eval, float(t_eval_hint[0]) + k * float(t_eval_hint[1])))
        desc.t_eval_exact = int(bool(t_eval_exact))


def _auto_order(model, mlp_width, prot_of_traj, P, B, traj_per_image):
    """launch_order="auto" before any composition: protocol-major order, or None.  One trajectory per lane (64 per wavefront) from
    these batch sizes on -- the dispatcher's crossovers (csrc/ionode_plan.hpp lane_wise_from): there the 64 lanes of a wavefront
    should read ONE protocol."""
    lane_from = int(lib().ionode_lane_wise_from(int(model), int(mlp_width or 0)))
    if lane_from > 0 and prot_of_traj is not None and P > 1 and B >= lane_from and not traj_per_image:
        return _protocol_major(prot_of_traj)
    return None


def _outputs(out, desc, shape, sdt, dev, states, current, stats, sse_ref, objective):
    """The output tensors, from `out` where the caller passed them, else allocated: (y, sse, i, status, stats, stats came from the
    caller).  The fused objective's pointers go into `desc`."""
    B, Nt, D, P = shape
    if out is None:
        out = {}
    y = out.get("y")
    if y is None and states:
        y = torch.empty((B, Nt, D), dtype=sdt, device=dev)
    sse = None
    if sse_ref is not None:  # fused objective: [P, Nt] reference currents -> per-trajectory sum of squared (absolute) residuals
        _dev_ptr(sse_ref, torch.float64, "sse_ref", (P, Nt))
        sse = out.get(objective)
        if sse is None:
            sse = torch.empty((B,), dtype=torch.float64, device=dev)
        desc.sse_ref, desc.sse_out = sse_ref.data_ptr(), sse.data_ptr()
    elif not states:
        raise IonodeError("states=False needs sse_ref (something must be computed)")
    i_out = out.get("i")
    if current and i_out is None:
        i_out = torch.empty((B, Nt), dtype=torch.float64, device=dev)
    status = out.get("status")
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=dev)
    st = out.get("stats")
    stats_from_caller = st is not None
    if stats and st is None:
        st = torch.empty((B, 4), dtype=torch.int64, device=dev)
    return y, sse, i_out, status, st, stats_from_caller


def _voltage_table(desc, v_at_outputs, prot_v, prot_t, t_eval, s):
    """Closed-form current / objective epilogue: V(t_k) once per protocol instead of once per trajectory per sample ("auto": when
    every protocol serves at least four trajectories; a [P, Nt] f64 tensor from an earlier call may be passed back in).  The table,
    also set in `desc`, or None."""
    vtab = None
    if isinstance(v_at_outputs, str):
        if 4 * desc.n_prot <= desc.n_traj:
            vtab = protocol_at_outputs(desc, prot_v, prot_t, t_eval, stream=s)
    else:
        vtab = v_at_outputs
        _dev_ptr(vtab, torch.float64, "v_at_outputs", (desc.n_prot, desc.n_out))
    if vtab is not None:
        desc.v_at_outputs = vtab.data_ptr()
    return vtab


def _compose(desc, cost_hint, tile_waves, want_current, caller_stats, pilot):
    """Shrink-aware tile composition: an order made on the device, on the current stream, ahead of the solve.  (launch order, also set
    in `desc`, and where its cost came from), or (None, None).  caller_stats: the `stats` tensor that `out=` carried, or None;
    pilot: the arguments of the pilot solve.

    cost_hint: where the cost comes from when compose_plan() says the launch qualifies (the lean N = 200 16-tile at one tile per
    compute unit; 4 heaviest + 12 lightest per tile, ionode_compose_order): a 1-D fp64 / int64 device tensor [B] gives explicit
    costs, "auto" (dopri5's default) reads the RHS evaluations of an earlier call from caller_stats (a training loop re-solves the
    same batch with slowly changing weights) and otherwise runs a pilot first -- the HH 2-state model on the same protocols, two
    output times, loose tolerance.  "hint" and "pilot" ask for one of the two by name; "auto" composes only the dispatcher's own
    16-tile (tile_waves = 0), the others also a forced one.  A stale or wrong cost changes the time, never the results.
    IONODE_COMPOSE=0|pilot|hint in the environment restricts the source."""
    cp = compose_plan(desc, want_current)
    if not cp["compose"]:
        return None, None
    B = desc.n_traj
    # "auto" follows the dispatcher's own choice of the tile only: a forced tile_waves pins the schedule (tuning runs and tests
    # that read per-tile effects back rely on index tiles); "pilot" / "hint" / a tensor ask for the composition explicitly
    want = cost_hint if not (isinstance(cost_hint, str) and cost_hint == "auto" and tile_waves) else None
    cost = composed = None
    if isinstance(want, torch.Tensor):
        if tuple(want.shape) != (B,):
            raise IonodeError(f"cost_hint: expected shape {(B,)}, got {tuple(want.shape)}")
        cost, composed = want, "explicit"
    elif want is not None and want not in ("auto", "pilot", "hint"):
        raise IonodeError("cost_hint: None, 'auto', 'pilot', 'hint' or a device tensor [B]")
    elif want in ("auto", "hint") and cp["source"] in ("hint", "auto") and caller_stats is not None \
            and _dev_ptr(caller_stats, torch.int64, "stats", (B, 4)):
        cost, composed = caller_stats[:, 2], "hint"
    elif want in ("auto", "pilot") and cp["source"] in ("pilot", "auto"):
        t_eval = pilot.pop("t_eval")
        run = dopri5(MODEL_HH2, pilot.pop("params"), pilot.pop("prot_v"), pilot.pop("y0"), torch.stack((t_eval[0], t_eval[desc.n_out - 1])),
                     rtol=PILOT_RTOL, atol=PILOT_ATOL, t_eval_hint=None, max_total_steps=PILOT_MAX_ATTEMPTS, launch_order=None,
                     cost_hint=None, **pilot)
        cost, composed = run["stats"][:, 2], "pilot"
    if cost is None:
        return None, None
    launch_order = compose_order(cost)
    desc.launch_order = launch_order.data_ptr()
    return launch_order, composed


def _record_workspace(desc, want_current, workspace, dev):
    """Deferred dense output: the record workspace -- the caller's (uint8, at least dense_defer_plan's bytes, 16-byte aligned: a caller
    that wants to read the record counts back keeps it), or one from torch's caching allocator (repeat calls cost nothing) -- or None
    when the plan defers nothing."""
    plan = dense_defer_plan(desc, want_current)
    if plan["capacity"] == 0:
        return None
    if workspace is None:
        return torch.empty((plan["workspace_bytes"],), dtype=torch.uint8, device=dev)
    _dev_ptr(workspace, torch.uint8, "workspace")
    if workspace.numel() < plan["workspace_bytes"]:
        raise IonodeError(f"workspace: {workspace.numel()} bytes, the plan asks for {plan['workspace_bytes']}")
    return workspace


def dopri5(model, params, prot_v, y0, t_eval, *, mlp_packed=None, mlp_layers=0, mlp_width=0, prot_t=None,
           prot_t0=0.0, prot_dt=1.0, prot_of_traj=None, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0,
           max_total_steps=0, max_step=0.0, ckpt=None, current=False, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, tile_waves=0, stats=True,
           step_log=None, t_eval_hint="auto", t_eval_exact=None, sse_ref=None, states=True, out=None, stream=None,
           v_at_outputs="auto", traj_per_image=0, launch_order="auto", workspace=None, cost_hint="auto", objective="sse"):
    """Launch one batched solve.  Every tensor lives on the current HIP device.

    launch_order: None (index order), an int32 device permutation [B] (ionode_desc.launch_order: slot s integrates trajectory
    order[s]; results stay at the trajectories' own indices, bit-identical to index order), or "auto": protocol-major order for
    the one-trajectory-per-lane kernels when several protocols are interleaved (the 64 lanes of a wavefront then interpolate
    one protocol instead of 64: -5 % on 393 216 HH trajectories over 64 protocols).

    cost_hint: where launch_order="auto" takes the cost of the shrink-aware tile composition from (_compose): None, "auto", "pilot",
    "hint" or a device tensor [B].  workspace: optional uint8 device tensor for the deferred dense output (_record_workspace).

    params [B, n_params] f64, prot_v [P, Np] f64, y0 [B, D] f32|f64 (selects the state dtype),
    t_eval [Nt] f64.  Returns dict(y [B, Nt, D], i [B, Nt] | None, status [B] i32, stats [B, 4] i64 | None);
    asynchronous on the current stream.

    objective: the kind of the fused objective that sse_ref asks for.  "sse" (default): sum_k (i_k - ref_k)^2 per trajectory under
    "sse".  "sae": sum_k |i_k - ref_k| under "sae" ("sse" is then None) -- Nt times the reference's prediction loss
    torch.mean(torch.abs(pred_yo - data)); same kernels, same summation order, inf for a failed trajectory.  With its gradient:
    grad.sum_of_abs.
    """
    kind = objective_kind(objective)
    if kind == OBJECTIVE_SAE and sse_ref is None:
        raise IonodeError("objective='sae' needs sse_ref (the reference currents [P, Nt])")
    if not torch.cuda.is_available():
        raise IonodeError("no HIP device visible: ionode has no CPU fallback")
    B, D = y0.shape
    Nt = t_eval.shape[0]
    P, Np = prot_v.shape
    sdt = y0.dtype
    if sdt not in (torch.float32, torch.float64):
        raise IonodeError("y0 must be float32 or float64")
    desc = make_desc(model=model, state_f32=int(sdt == torch.float32), n_state=D, n_out=Nt, n_traj=B, n_prot=P,
                     prot_n=Np, mlp_layers=mlp_layers, mlp_width=mlp_width, n_params=params.shape[1],
                     max_steps=max_steps, max_total_steps=max_total_steps, max_step=max_step, prot_t0=prot_t0, prot_dt=prot_dt, v_oob=v_oob, rtol=rtol, atol=atol,
                     obs_g=obs_g, obs_e=obs_e, obs_open_state_only=int(obs_open_state_only), tile_waves=tile_waves)
    if traj_per_image:  # several weight images: mlp_packed [n_images, floats], trajectory b uses image b // traj_per_image
        if mlp_packed is None or mlp_packed.dim() != 2 or mlp_packed.shape[0] * traj_per_image < B or not mlp_packed.is_contiguous():
            raise IonodeError("traj_per_image needs a contiguous mlp_packed [n_images, floats] with n_images * traj_per_image >= B")
        desc.mlp_image_stride, desc.traj_per_image = int(mlp_packed.shape[1]), int(traj_per_image)
    _grid_hint(desc, t_eval, t_eval_hint, t_eval_exact)
    auto_order = isinstance(launch_order, str)
    if auto_order:
        if launch_order != "auto":
            raise IonodeError("launch_order: None, 'auto' or an int32 device tensor [B]")
        launch_order = _auto_order(model, mlp_width, prot_of_traj, P, B, traj_per_image)
    if launch_order is not None:
        _dev_ptr(launch_order, torch.int32, "launch_order", (B,))
        desc.launch_order = launch_order.data_ptr()
    if ckpt is not None:  # [B, cap, record] f64 device tensor: accepted-step records for the backward sweep
        _dev_ptr(ckpt, torch.float64, "ckpt", (B, ckpt.shape[1], ckpt_record_doubles(D)))
        desc.ckpt = ckpt.data_ptr()
        desc.ckpt_cap = ckpt.shape[1]
    if step_log is not None:  # [cap, 4] f64 device tensor: (t0, dt, ratio, accepted) per attempt of trajectory 0
        _dev_ptr(step_log, torch.float64, "step_log")
        desc.step_log = step_log.data_ptr()
        desc.step_log_cap = step_log.shape[0]
    dev = y0.device
    y, sse, i_out, status, st, stats_from_caller = _outputs(out, desc, (B, Nt, D, P), sdt, dev, states, current, stats, sse_ref, objective)
    s = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    vtab = None
    if (current or sse_ref is not None) and model in (MODEL_HH2, MODEL_MARKOV6) and v_at_outputs is not None:
        vtab = _voltage_table(desc, v_at_outputs, prot_v, prot_t, t_eval, s)
    # the composition's and the record workspace's buffers come from torch's caching allocator and go back to it when this call
    # returns -- in stream order, which holds for torch's current stream only, so a foreign stream composes and defers nothing
    composed = None
    if auto_order and launch_order is None and cost_hint is not None and stream is None and prot_t is None and Nt >= 2:
        pilot = dict(params=params, prot_v=prot_v, y0=y0, t_eval=t_eval, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=prot_of_traj, v_oob=v_oob)
        launch_order, composed = _compose(desc, cost_hint, tile_waves, i_out is not None, st if stats_from_caller else None, pilot)
    ws = None
    if stream is None and prot_t is None and y is not None:
        ws = _record_workspace(desc, i_out is not None, workspace, dev)
    rc = lib().ionode_dopri5_objective(   # kind 0 is ionode_dopri5_composed by definition: one call site
        C.byref(desc),
        _dev_ptr(mlp_packed, torch.float32, "mlp_packed"),
        _dev_ptr(params, torch.float64, "params", (B, params.shape[1])),
        _dev_ptr(prot_v, torch.float64, "prot_v"),
        _dev_ptr(prot_t, torch.float64, "prot_t", (Np,)) if prot_t is not None else None,
        _dev_ptr(prot_of_traj, torch.int32, "prot_of_traj", (B,)) if prot_of_traj is not None else None,
        _dev_ptr(y0, sdt, "y0"),
        _dev_ptr(t_eval, torch.float64, "t_eval"),
        _dev_ptr(y, sdt, "y_out", (B, Nt, D)) if y is not None else None,
        _dev_ptr(i_out, torch.float64, "i_out", (B, Nt)) if i_out is not None else None,
        _dev_ptr(status, torch.int32, "status", (B,)),
        _dev_ptr(st, torch.int64, "stats", (B, 4)) if st is not None else None,
        C.c_void_p(s),
        C.c_void_p(ws.data_ptr()) if ws is not None else None,
        ws.numel() if ws is not None else 0,
        COST_SOURCE[composed],
        kind,
    )
    if rc != 0:
        raise IonodeError(f"ionode_dopri5 failed ({rc}): {last_error()}")
    return {"y": y, "i": i_out, "status": status, "stats": st, "sse": sse if kind == OBJECTIVE_SSE else None,
            "sae": sse if kind == OBJECTIVE_SAE else None, "desc": desc, "v_at_outputs": vtab,
            "launch_order": launch_order, "composed": composed, "kernel": lib().ionode_last_kernel_name().decode()}


def uniform_grid(t_eval):
    """(t0, dt, largest |t_k - (t0 + k dt)|) of an output grid that is uniform -- dt > 0 from the end points, every t_k within dt / 2 of
    its place -- or None.  One small device->host read."""
    n = int(t_eval.shape[0])
    if n < 2:
        return None
    t0 = t_eval[0]
    dt = (t_eval[n - 1] - t0) / (n - 1)
    dev = (t_eval - (t0 + torch.arange(n, dtype=torch.float64, device=t_eval.device) * dt)).abs().max()
    t0, dt, dev = (float(x) for x in torch.stack([t0, dt, dev]).cpu())
    return (t0, dt, dev) if dt > 0 and dev <= 0.5 * dt else None


def sweep_launch(name, desc, it_begin, it_end, n_iter, stream, kind=None, **buffers):
    """Call the backward-sweep entry point `name` on iterations [it_begin, it_end) with its buffers BY NAME: exactly the names of
    SWEEP_BUFFERS[name], each a device tensor or None (NULL); `stream` is a torch stream.  With `kind` (OBJECTIVE_SSE | OBJECTIVE_SAE)
    `name` is an entry point of OBJECTIVE_BUFFERS, which takes the kind behind the descriptor.  Raises IonodeError with the return code
    and ionode_grad_last_error()."""
    names = (SWEEP_BUFFERS if kind is None else OBJECTIVE_BUFFERS)[name]
    if set(buffers) != set(names):
        raise TypeError(f"{name}: missing {sorted(set(names) - set(buffers))}, unknown {sorted(set(buffers) - set(names))}")
    ptrs = [None if buffers[n] is None else C.c_void_p(buffers[n].data_ptr()) for n in names]
    head = () if kind is None else (int(kind),)
    rc = getattr(lib(), name)(C.byref(desc), *head, it_begin, it_end, n_iter, *ptrs, C.c_void_p(stream.cuda_stream))
    if rc != 0:
        raise IonodeError(f"{name} failed ({rc}): {lib().ionode_grad_last_error().decode()}")


def objective_launch(name, desc, kind, it_begin, it_end, n_iter, stream, **buffers):
    """sweep_launch for the entry points of OBJECTIVE_BUFFERS: the same named-buffer call, the same error."""
    sweep_launch(name, desc, it_begin, it_end, n_iter, stream, kind=int(kind), **buffers)


def protocol_at_outputs(desc, prot_v, prot_t, t_eval, stream=None):
    """[P, Nt] f64: every protocol's voltage at the output times (ionode_protocol_at_outputs), on prot_v's device."""
    out = torch.empty((desc.n_prot, desc.n_out), dtype=torch.float64, device=prot_v.device)
    s = stream if stream is not None else torch.cuda.current_stream(prot_v.device).cuda_stream
    rc = lib().ionode_protocol_at_outputs(C.byref(desc), _dev_ptr(prot_v, torch.float64, "prot_v"),
                                          _dev_ptr(prot_t, torch.float64, "prot_t") if prot_t is not None else None,
                                          _dev_ptr(t_eval, torch.float64, "t_eval"), out.data_ptr(), C.c_void_p(s))
    if rc != 0:
        raise IonodeError(f"ionode_protocol_at_outputs failed ({rc}): {last_error()}")
    return out
