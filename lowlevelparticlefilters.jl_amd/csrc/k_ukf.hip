// k_ukf.hip — k_ukf, k_ukf_smooth (kernels/ukf.hpp): banks of unscented Kalman filters (llpf_ukf_bank_run, llpf_ukf_bank_smooth).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here and nowhere
// else, for both kernels, by dispatch_builtin_model (kernels/dispatch.hpp).  A run-time compiled model (a user snippet, a traced callable,
// the linear-Gaussian model above 4 states) gets its k_ukf from a program of its own (engine.hpp: JitProgram; kernels/jit_bank.hpp),
// compiled on the first bank of that model and cached per model — the program of llpf_model_compile is left as it is — and its
// k_ukf_smooth, with the posterior-storing k_ukf<..., true> of the smoother's forward pass, from another one, compiled on the first smooth
// of that model and cached in an entry of its own: a bank that never smooths compiles what it always did.
#include "engine.hpp"
#include "shared/llpf_ukf.h"
#include "jit_ukf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/ukf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_ukf_t(const ModelD* models, const UkfArgs& a, hipStream_t s) {
    if (a.post)
        hipLaunchKernelGGL((k_ukf<Model, NX, NY, true>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    else
        hipLaunchKernelGGL((k_ukf<Model, NX, NY, false>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
template <class Model, int NX>
static hipError_t launch_ukf_smooth_t(const ModelD* models, const UkfSmoothArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_ukf_smooth<Model, NX>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// The forward and the backward kernel are entries of their own.  Kernel 0: k_ukf<UserModel, nx, ny> of a forward entry,
// k_ukf_smooth<UserModel, nx> of a smoother's (":smooth"); kernel 1 of a smoother's entry: k_ukf<UserModel, nx, ny, true>, its forward pass
static JitCache g_ukf;

// compiles k_ukf (smooth = false), or k_ukf_smooth and the posterior-storing k_ukf<..., true> (smooth = true), of a run-time compiled
// model unless its entry exists
static int ukf_compile(int model_id, int nx, int ny, bool smooth, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_ukf.prepare(jit_bank_key(model_id, nx, ny, smooth ? ":smooth" : ""), [&]() {
        const std::string dims = std::to_string(nx) + ", " + std::to_string(ny);
        std::vector<std::string> exprs = {"llpf::k_ukf<llpf::UserModel, " + dims + ">"};
        if (smooth) exprs = {"llpf::k_ukf_smooth<llpf::UserModel, " + std::to_string(nx) + ">", "llpf::k_ukf<llpf::UserModel, " + dims + ", true>"};
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_UKF_SHARED, LLPF_JIT_UKF, "llpf_user_ukf.hip", exprs,
                              smooth ? "hiprtc (k_ukf_smooth): " : "hiprtc (k_ukf): ", err);
    });
}
int ukf_prepare(int model_id, int nx, int ny, std::string& err) { return ukf_compile(model_id, nx, ny, false, err); }
int ukf_smooth_prepare(int model_id, int nx, int ny, std::string& err) { return ukf_compile(model_id, nx, ny, true, err); }

hipError_t launch_ukf(int model_id, int nx, int ny, const ModelD* models, const UkfArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny))      // with a.post: the smoother's forward kernel k_ukf<..., true>
        return jit_bank_launch(g_ukf, jit_bank_key(model_id, nx, ny, a.post ? ":smooth" : ""), a.post ? 1 : 0, models, a, a.F, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_ukf_t<typename M::Model, M::NX, M::NY>(models, a, s);
    });
}

hipError_t launch_ukf_smooth(int model_id, int nx, int ny, const ModelD* models, const UkfSmoothArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) return jit_bank_launch(g_ukf, jit_bank_key(model_id, nx, ny, ":smooth"), 0, models, a, a.F, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_ukf_smooth_t<typename M::Model, M::NX>(models, a, s);
    });
}

}  // namespace llpf
