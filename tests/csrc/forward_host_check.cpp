// forward_host_check.cpp -- stand-alone driver of the forward path's HOST code (csrc/ionode_plan.hpp, ionode_pack.hpp and
// checked_solve in ionode_capi.hip) for a host sanitizer build.  It launches nothing: every solve call below is one the checks refuse.
//   hipcc <csrc/Makefile's FLAGS> -Xarch_host -fsanitize=address,undefined -c csrc/ionode_capi.hip -o capi_san.o
//   clang++ -std=c++17 -fsanitize=address,undefined -I include -c tests/csrc/forward_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined capi_san.o main.o <the library's other eight objects> -o check && ./check
// (never loaded into python, never run on a GPU machine: profiles/forward_plan_refactor.md has the result)
#include <cstdio>
#include <cstring>
#include <vector>

#include "ionode.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, ionode_last_error()); } } while (0)

static ionode_desc desc(int model, int f32, int n_traj, int n_out, int width) {
  ionode_desc d;
  memset(&d, 0, sizeof d);
  d.model = model; d.state_f32 = f32; d.n_state = model == IONODE_MODEL_MARKOV6 ? 6 : 2; d.n_out = n_out; d.n_traj = n_traj; d.n_prot = 1;
  d.prot_n = 100; d.mlp_layers = width ? 5 : 0; d.mlp_width = width; d.n_params = d.n_state == 6 ? 12 : 8; d.prot_dt = 0.1; d.rtol = 1e-7;
  d.atol = 1e-9; d.t_eval_dt_hint = 0.5; d.t_eval_exact = 1;
  return d;
}

int main() {
  // the ten shapes of tests/golden/make_dispatch_fixture.py PACK_SHAPES
  const int shapes[10][2] = {{0, 10}, {5, 10}, {3, 16}, {2, 17}, {1, 64}, {5, 100}, {5, 200}, {10, 200}, {1, 300}, {2, 500}};
  for (const auto &s : shapes) {
    const int L = s[0], N = s[1];
    std::vector<float> w((size_t)2 * N + N + (size_t)L * ((size_t)N * N + N) + N + 1);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)(i % 97) - 48.0f;
    std::vector<float> img(ionode_mlp_packed_floats(L, N));   // exactly the size asked for: a write past it is the sanitizer's to find
    EXPECT(!img.empty() && ionode_mlp_pack(w.data(), L, N, img.data()) == IONODE_OK);
  }
  EXPECT(ionode_mlp_packed_floats(1, 513) == 0 && ionode_mlp_pack(nullptr, 1, 10, nullptr) == IONODE_ERR_ARG);
  // the six plan queries
  const ionode_desc ds[] = {desc(IONODE_MODEL_NNF, 0, 4096, 20001, 200), desc(IONODE_MODEL_NND, 1, 257, 65, 200), desc(IONODE_MODEL_NNF, 0, 64, 1000, 100),
                            desc(IONODE_MODEL_HH2, 0, 65536, 1000, 0), desc(IONODE_MODEL_MARKOV6, 1, 64, 2, 0)};
  for (const ionode_desc &d : ds) {
    int32_t geo[4], cp[2];
    int64_t p[2];
    EXPECT(ionode_launch_geometry(&d, geo) == IONODE_OK && geo[0] > 0 && ionode_kernel_name(&d)[0] != '\0');
    for (int want = 0; want < 2; ++want) {
      EXPECT(ionode_dense_defer_plan(&d, want, p) == IONODE_OK && ionode_dense_tail_plan(&d, want, p) == IONODE_OK);
      EXPECT(ionode_compose_tail_plan(&d, want, 2, p) == IONODE_OK && ionode_compose_tail_plan(&d, want, 3, p) == IONODE_ERR_ARG);
      EXPECT(ionode_compose_plan(&d, want, cp) == IONODE_OK);
    }
  }
  int32_t geo[4];
  EXPECT(ionode_launch_geometry(nullptr, geo) == IONODE_ERR_ARG && ionode_kernel_name(nullptr)[0] == '\0');
  // each solve entry point: NULL descriptor, and one refused defect (no params; host stand-in for the other pointers)
  double buf[8] = {0};
  void *p = buf;
  const ionode_desc d = desc(IONODE_MODEL_HH2, 0, 4, 8, 0);
  const float *no_mlp = nullptr;
  const double *b = buf, *no_params = nullptr;
#define SOLVE_ARGS(dd, params) dd, no_mlp, params, b, nullptr, nullptr, p, b, p, nullptr, (int32_t *)p, nullptr, nullptr
  EXPECT(ionode_dopri5(SOLVE_ARGS(nullptr, b)) == IONODE_ERR_ARG && !strcmp(ionode_last_error(), "null descriptor"));
  EXPECT(ionode_dopri5_deferred(SOLVE_ARGS(nullptr, b), p, 64) == IONODE_ERR_ARG && !strcmp(ionode_last_error(), "null descriptor"));
  EXPECT(ionode_dopri5_composed(SOLVE_ARGS(nullptr, b), p, 64, 0) == IONODE_ERR_ARG && !strcmp(ionode_last_error(), "null descriptor"));
  EXPECT(ionode_dopri5_objective(SOLVE_ARGS(nullptr, b), p, 64, 0, 0) == IONODE_ERR_ARG && !strcmp(ionode_last_error(), "null descriptor"));
  EXPECT(ionode_dopri5_objective(SOLVE_ARGS(nullptr, b), p, 64, 0, 1) == IONODE_ERR_ARG);
  EXPECT(ionode_dopri5(SOLVE_ARGS(&d, no_params)) == IONODE_ERR_ARG);
  EXPECT(ionode_dopri5_deferred(SOLVE_ARGS(&d, no_params), p, 64) == IONODE_ERR_ARG);
  EXPECT(ionode_dopri5_composed(SOLVE_ARGS(&d, b), p, 64, 9) == IONODE_ERR_ARG);
  EXPECT(ionode_dopri5_objective(SOLVE_ARGS(&d, b), p, 64, 0, 2) == IONODE_ERR_ARG);
  EXPECT(ionode_protocol_at_outputs(nullptr, b, nullptr, b, buf, nullptr) == IONODE_ERR_ARG);
  printf("forward_host_check: %d failure(s)\n", failures);
  return failures != 0;
}
