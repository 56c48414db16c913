// k_aukf.hip — k_aukf (kernels/aukf.hpp): banks of unscented Kalman filters with augmented process noise (llpf_aukf_bank_run).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here for k_aukf
// and nowhere else, by dispatch_builtin_model (kernels/dispatch.hpp); they have no dynamics_w and take the additive path.  A run-time
// compiled model (a user snippet or a traced callable, with or without dynamics_w; the linear-Gaussian model above 4 states) gets its
// k_aukf from a program of its own (engine.hpp: JitProgram; kernels/jit_bank.hpp), compiled on the first such bank of that model and
// cached per (model id, nx, ny); the programs of the other units are left as they are.
#include "engine.hpp"
#include "shared/llpf_aukf.h"
#include "jit_aukf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/aukf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_aukf_t(const ModelD* models, const AukfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_aukf<Model, NX, NY>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
// ---- run-time compiled models (kernels/jit_bank.hpp) ----  Kernel 0: k_aukf<UserModel, nx, ny>
static JitCache g_aukf;

int aukf_prepare(int model_id, int nx, int ny, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_aukf.prepare(jit_bank_key(model_id, nx, ny, ""), [&]() {
        const std::string expr = "llpf::k_aukf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ">";
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_AUKF_SHARED, LLPF_JIT_AUKF, "llpf_user_aukf.hip", {expr}, "hiprtc (k_aukf): ", err);
    });
}

hipError_t launch_aukf(int model_id, int nx, int ny, const ModelD* models, const AukfArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) return jit_bank_launch(g_aukf, jit_bank_key(model_id, nx, ny, ""), 0, models, a, a.F, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_aukf_t<typename M::Model, M::NX, M::NY>(models, a, s);
    });
}

}  // namespace llpf
