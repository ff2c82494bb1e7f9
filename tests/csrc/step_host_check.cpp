// step_host_check.cpp -- stand-alone driver of the optimiser steps' HOST code (csrc/ionode_step_capi.hpp, the three *_capi.hip units, the
// one refuse() of ionode_grad_capi.hip and the host mirrors behind ionode_lm_step_host / ionode_cmaes_step_host / ionode_mcmc_step_host)
// for a host sanitizer build.  It launches nothing: every call is a host mirror's or one the checks refuse.
//   for u in ionode_grad_capi ionode_lm_capi ionode_cmaes_capi ionode_mcmc_capi inst_lm inst_cmaes inst_mcmc:
//     hipcc <csrc/Makefile's FLAGS of that unit> -Xarch_host -fsanitize=address,undefined -c csrc/$u.hip -o ${u}_san.o
//   clang++ -std=c++17 -fsanitize=address,undefined -I include -c tests/csrc/step_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined *_san.o main.o <the library's other nine objects> -o check && ./check
// (never loaded into python, never run on a GPU machine: profiles/step_refactor.md has the result)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ionode.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, ionode_grad_last_error()); } } while (0)

constexpr int K = 2, P = 1, NF = 2, NPAR = 8;

// the box of a tiny problem: two free parameters of eight, log parameters, 0.1 .. 10
template <class Desc>
static void box(Desc &d) {
  d.n_active = K; d.n_prot = P; d.n_params = NPAR; d.n_free = NF; d.log_parameters = 1; d.max_iter = 5;
  for (int j = 0; j < NF; ++j) { d.free_idx[j] = j; d.lo[j] = 0.1; d.hi[j] = 10.0; }
  for (int i = 0; i < NPAR; ++i) d.base[i] = 1.0 + 0.1 * i;
}

static bool is(const char *text) { return strcmp(ionode_grad_last_error(), text) == 0; }

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<int32_t> status(64, 0), flag(K, 0), iters(2 * K, 0);
  std::vector<double> trial(64 * NPAR, 1.0), value(64, 1.0);

  {   // Levenberg-Marquardt: state = f, lam, nu, pred, then u, x, g, ut, xt, delta [nf], H [nf][nf]
    ionode_lm_desc d;
    memset(&d, 0, sizeof d);
    box(d);
    d.n_cand = K; d.gtol = d.xtol = d.ftol = 1e-8; d.rho_accept = 1e-4; d.lam_max = 1e16;
    const int words = IONODE_LM_STATE_U + 6 * NF + NF * NF;
    std::vector<double> state(K * words, 0.0), jtr(K * P * NPAR, 0.5), jtj(K * P * NPAR * NPAR, 0.0);
    for (int c = 0; c < K; ++c) {
      state[c * words + IONODE_LM_STATE_F] = inf; state[c * words + IONODE_LM_STATE_LAM] = 1e-3; state[c * words + IONODE_LM_STATE_NU] = 2.0;
      for (int j = 0; j < NF; ++j) state[c * words + IONODE_LM_STATE_U + NF + j] = state[c * words + IONODE_LM_STATE_U + 4 * NF + j] = 1.0;   // x, xt (u = ut = 0)
    }
    for (int r = 0; r < K * P; ++r) for (int i = 0; i < NPAR; ++i) jtj[(r * NPAR + i) * NPAR + i] = 1.0;
    EXPECT(ionode_lm_step_host(&d, nullptr, value.data(), jtr.data(), jtj.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_OK);
    EXPECT(iters[0] == 1 && iters[2] == 1);
    d.lo[1] = 20.0;
    EXPECT(ionode_lm_step_host(&d, nullptr, value.data(), jtr.data(), jtj.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_lm_step_host: bounds of free parameter 1: lo > hi (or NaN)"));
    d.lo[1] = 0.1; d.n_free = 13;
    EXPECT(ionode_lm_step_host(&d, nullptr, value.data(), jtr.data(), jtj.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_lm_step_host: n_free = 13 outside 1 .. 12"));
  }

  {   // CMA-ES, lambda = 4: the first call samples generation 0 and reads no value
    ionode_cmaes_desc d;
    memset(&d, 0, sizeof d);
    box(d);
    const int lam = 4;
    d.n_run = K; d.lambda = lam; d.unchanged_iters = 100; d.unchanged_threshold = 1e-3; d.tolx = 1e-11; d.seed = 7;
    const int words = IONODE_CMAES_STATE_M + 8 * NF + 3 * NF * NF + 2 * lam + 2 * lam * NF;
    std::vector<double> state(K * words, 0.0);
    for (int c = 0; c < K; ++c) {
      double *st = state.data() + c * words;
      st[IONODE_CMAES_STATE_SIGMA] = 0.1;
      for (int j = 0; j < NF; ++j) {
        st[IONODE_CMAES_STATE_M + 4 * NF + j] = 1.0;                       // D
        st[IONODE_CMAES_STATE_M + 5 * NF + j] = 1.0;                       // best x
        st[IONODE_CMAES_STATE_M + 8 * NF + j * NF + j] = 1.0;              // C
        st[IONODE_CMAES_STATE_M + 8 * NF + NF * NF + j * NF + j] = 1.0;    // B
      }
    }
    flag.assign(K, 0); iters.assign(2 * K, 0);
    EXPECT(ionode_cmaes_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_OK);
    EXPECT(ionode_cmaes_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_OK);
    d.lo[0] = 0.0;
    EXPECT(ionode_cmaes_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_cmaes_step_host: log_parameters needs positive bounds (free parameter 0)"));
    d.lo[0] = 0.1;
    EXPECT(ionode_cmaes_step_host(&d, nullptr, value.data(), status.data(), nullptr, flag.data(), iters.data(), trial.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_cmaes_step_host: required buffer is NULL (value, status, state, flag, iters, trial)"));
  }

  {   // adaptive Metropolis, fixed sigma: state = 4 scalars, u, ut, x, xt, mu [n], C and L [n][n]
    ionode_mcmc_desc d;
    memset(&d, 0, sizeof d);
    box(d);
    d.n_chain = K; d.sigma = 0.1; d.adapt_start = 1; d.thin = 1; d.sample_cap = 6; d.seed = 7; d.n_samples = 10.0; d.eta = 0.6; d.target_accept = 0.234;
    d.epsilon = 1e-12;
    const int words = IONODE_MCMC_STATE_U + 5 * NF + 2 * NF * NF;
    std::vector<double> state(K * words, 0.0), samples(K * d.sample_cap * (NF + 1), 0.0);
    for (int c = 0; c < K; ++c) {
      double *st = state.data() + c * words;
      for (int j = 0; j < NF; ++j) {
        st[IONODE_MCMC_STATE_U + 2 * NF + j] = st[IONODE_MCMC_STATE_U + 3 * NF + j] = 1.0;   // x, xt (u = ut = mu = 0)
        st[IONODE_MCMC_STATE_U + 5 * NF + j * NF + j] = 1.0;                                   // C
      }
    }
    flag.assign(K, 0); iters.assign(2 * K, 0);
    for (int it = 0; it < 3; ++it)
      EXPECT(ionode_mcmc_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data(), samples.data()) == IONODE_OK);
    EXPECT(iters[0] == 3 && iters[2] == 3);
    d.free_idx[1] = NPAR;
    EXPECT(ionode_mcmc_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data(), samples.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_mcmc_step_host: free index 8 outside the model's 8 parameters"));
    d.free_idx[1] = 1; d.hi[0] = inf;
    EXPECT(ionode_mcmc_step_host(&d, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data(), samples.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_mcmc_step_host: infinite bound of free parameter 0 (the box is the prior: it must be finite)"));
    EXPECT(ionode_mcmc_step_host(nullptr, nullptr, value.data(), status.data(), state.data(), flag.data(), iters.data(), trial.data(), samples.data()) == IONODE_ERR_ARG);
    EXPECT(is("ionode_mcmc_step_host: null descriptor"));
  }

  printf(failures ? "step_host_check: %d FAILED\n" : "step_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
