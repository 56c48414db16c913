// k_enkf.hip — k_enkf, k_enkf_init, k_enkf_moments (kernels/enkf.hpp): banks of ensemble Kalman filters (llpf_enkf_bank_*).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here and nowhere
// else, by dispatch_builtin_model (kernels/dispatch.hpp).  A run-time compiled model (a user snippet, with or without `noise` and `initial`
// members of its own, a traced callable, the linear-Gaussian model above 4 states) gets its k_enkf and k_enkf_init from a program of its
// own (engine.hpp: JitProgram; kernels/jit_bank.hpp), compiled on the first bank of that model and cached per (model id, nx, ny) — the
// programs of llpf_model_compile, k_simulate, k_ukf and k_ekf are left as they are.  k_enkf_moments knows no model: nx in 1..8 is here.
#include "engine.hpp"
#include "shared/llpf_enkf.h"
#include "jit_enkf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/enkf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

// one workgroup per ensemble
static dim3 enkf_grid(int64_t F) { return dim3((unsigned)F, 1, 1); }
static dim3 enkf_init_grid(int64_t F, int N) { return dim3((unsigned)((N + ENKF_BLOCK - 1) / ENKF_BLOCK), (unsigned)F, 1); }

// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// Kernel 0: k_enkf<UserModel, nx, ny>; kernel 1: k_enkf_init<UserModel, nx>
static JitCache g_enkf;

int enkf_prepare(int model_id, int nx, int ny, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_enkf.prepare(jit_bank_key(model_id, nx, ny, ""), [&]() {
        const std::string dims = std::to_string(nx) + ", " + std::to_string(ny);
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_ENKF_SHARED, LLPF_JIT_ENKF, "llpf_user_enkf.hip",
                              {"llpf::k_enkf<llpf::UserModel, " + dims + ">", "llpf::k_enkf_init<llpf::UserModel, " + std::to_string(nx) + ">"},
                              "hiprtc (k_enkf): ", err);
    });
}
// a kernel of such a program on a grid of its own (jit_bank_launch's is one thread per filter)
template <class Args>
static hipError_t enkf_jit_launch(const std::string& key, int which, dim3 grid, const ModelD* models, Args args, hipStream_t s) {
    hipFunction_t fn = nullptr;
    const hipError_t e = g_enkf.function(key, which, &fn);
    if (e != hipSuccess) return e;
    void* params[] = {&models, &args};
    return hipModuleLaunchKernel(fn, grid.x, grid.y, 1, ENKF_BLOCK, 1, 1, 0, s, params, nullptr);
}

hipError_t launch_enkf(int model_id, int nx, int ny, const ModelD* models, const EnkfArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) return enkf_jit_launch(jit_bank_key(model_id, nx, ny, ""), 0, enkf_grid(a.F), models, a, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        hipLaunchKernelGGL((k_enkf<typename M::Model, M::NX, M::NY>), enkf_grid(a.F), dim3(ENKF_BLOCK), 0, s, models, a);
        return hipGetLastError();
    });
}

hipError_t launch_enkf_init(int model_id, int nx, int ny, const ModelD* models, int F, const EnkfInitArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) return enkf_jit_launch(jit_bank_key(model_id, nx, ny, ""), 1, enkf_init_grid(F, a.N), models, a, s);
    // (the draw of a built-in model reads the descriptor's d0 alone: one instantiation per nx, under the model with ny = 1)
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        hipLaunchKernelGGL((k_enkf_init<QuadTank<4, 2>, 4>), enkf_init_grid(F, a.N), dim3(ENKF_BLOCK), 0, s, models, a);
        return hipGetLastError();
    }
    return dispatch_dim<1, 4>(nx, [&](auto NX) {
        hipLaunchKernelGGL((k_enkf_init<LinGauss<decltype(NX)::value, 1>, decltype(NX)::value>), enkf_init_grid(F, a.N), dim3(ENKF_BLOCK), 0, s, models, a);
        return hipGetLastError();
    });
}

hipError_t launch_enkf_moments(int nx, const double* members, double* state, int64_t F, int N, int zero_ll, hipStream_t s) {
    return dispatch_dim<1, LLPF_KF_MAXX>(nx, [&](auto NX) {
        hipLaunchKernelGGL((k_enkf_moments<decltype(NX)::value>), enkf_grid(F), dim3(ENKF_BLOCK), 0, s, members, state, F, N, zero_ll);
        return hipGetLastError();
    });
}

}  // namespace llpf
