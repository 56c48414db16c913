// k_ekf.hip — k_ekf (kernels/ekf.hpp): banks of extended and of iterated extended Kalman filters (llpf_ekf_bank_run).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here and nowhere
// else, for both kernels, by dispatch_builtin_model (kernels/dispatch.hpp).  A run-time compiled model (a user snippet or a traced
// callable with dynamics_jac and measurement_jac, the linear-Gaussian model above 4 states) gets its k_ekf from a program of its own
// (engine.hpp: JitProgram; kernels/jit_bank.hpp), compiled on the first bank of that model and cached per (model id, nx, ny) — the programs
// of llpf_model_compile, k_simulate and k_ukf are left as they are — and its iterated kernel k_ekf<..., IekfArgs> from another one,
// compiled on the first iterated use of that model and cached in an entry of its own: a bank that never iterates compiles what it always did.
#include "engine.hpp"
#include "shared/llpf_ekf.h"
#include "jit_ekf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/ekf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

// ia: null for the plain kernel, or the arguments of the iterated one, k_ekf<..., IekfArgs> (its EkfArgs part is `a`)
template <class Model, int NX, int NY>
static hipError_t launch_ekf_t(const ModelD* models, const EkfArgs& a, const IekfArgs* ia, hipStream_t s) {
    if (ia)
        hipLaunchKernelGGL((k_ekf<Model, NX, NY, IekfArgs>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, *ia);
    else
        hipLaunchKernelGGL((k_ekf<Model, NX, NY>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// The plain and the iterated kernel are entries of their own.  Kernel 0: k_ekf<UserModel, nx, ny>, or k_ekf<UserModel, nx, ny, IekfArgs>
// (":iterated")
static JitCache g_ekf;

// compiles k_ekf (iterated = false) or k_ekf<..., IekfArgs> (iterated = true) of a run-time compiled model unless its entry exists
static int ekf_compile(int model_id, int nx, int ny, bool iterated, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_ekf.prepare(jit_bank_key(model_id, nx, ny, iterated ? ":iterated" : ""), [&]() {
        const std::string expr = "llpf::k_ekf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + (iterated ? ", llpf::IekfArgs>" : ">");
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_EKF_SHARED, LLPF_JIT_EKF, "llpf_user_ekf.hip", {expr},
                              iterated ? "hiprtc (k_ekf, iterated): " : "hiprtc (k_ekf): ", err);
    });
}
int ekf_prepare(int model_id, int nx, int ny, std::string& err) { return ekf_compile(model_id, nx, ny, false, err); }
int iekf_prepare(int model_id, int nx, int ny, std::string& err) { return ekf_compile(model_id, nx, ny, true, err); }

static hipError_t launch_ekf_any(int model_id, int nx, int ny, const ModelD* models, const EkfArgs& a, const IekfArgs* ia, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) {
        const std::string key = jit_bank_key(model_id, nx, ny, ia ? ":iterated" : "");
        return ia ? jit_bank_launch(g_ekf, key, 0, models, *ia, a.F, s) : jit_bank_launch(g_ekf, key, 0, models, a, a.F, s);
    }
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_ekf_t<typename M::Model, M::NX, M::NY>(models, a, ia, s);
    });
}

hipError_t launch_ekf(int model_id, int nx, int ny, const ModelD* models, const EkfArgs& a, hipStream_t s) {
    return launch_ekf_any(model_id, nx, ny, models, a, nullptr, s);
}
hipError_t launch_iekf(int model_id, int nx, int ny, const ModelD* models, const EkfArgs& a, int32_t maxiters, double epsilon, hipStream_t s) {
    IekfArgs ia{};
    static_cast<EkfArgs&>(ia) = a;
    ia.maxiters = maxiters;
    ia.epsilon = epsilon;
    return launch_ekf_any(model_id, nx, ny, models, a, &ia, s);
}

}  // namespace llpf
