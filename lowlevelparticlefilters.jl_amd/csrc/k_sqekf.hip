// k_sqekf.hip — k_sqekf (kernels/sqekf.hpp): banks of square-root extended Kalman filters (llpf_sqekf_bank_run).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here for k_sqekf
// and nowhere else, by dispatch_builtin_model (kernels/dispatch.hpp).  A run-time compiled model (a user snippet or a traced callable
// with dynamics_jac and measurement_jac, the linear-Gaussian model above 4 states) gets its k_sqekf from a program of its own
// (engine.hpp: JitProgram; kernels/jit_bank.hpp), compiled on the first such bank of that model and cached per (model id, nx, ny); the
// programs of the other units are left as they are.
#include "engine.hpp"
#include "shared/llpf_sqekf.h"
#include "jit_sqekf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/sqekf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_sqekf_t(const ModelD* models, const KfModelArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_sqekf<Model, NX, NY>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
// ---- run-time compiled models (kernels/jit_bank.hpp) ----  Kernel 0: k_sqekf<UserModel, nx, ny>
static JitCache g_sqekf;

int sqekf_prepare(int model_id, int nx, int ny, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_sqekf.prepare(jit_bank_key(model_id, nx, ny, ""), [&]() {
        const std::string expr = "llpf::k_sqekf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ">";
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_SQEKF_SHARED, LLPF_JIT_SQEKF, "llpf_user_sqekf.hip", {expr}, "hiprtc (k_sqekf): ", err);
    });
}

hipError_t launch_sqekf(int model_id, int nx, int ny, const ModelD* models, const KfModelArgs& a, hipStream_t s) {
    if (!jit_bank_builtin(model_id, nx, ny)) return jit_bank_launch(g_sqekf, jit_bank_key(model_id, nx, ny, ""), 0, models, a, a.F, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_sqekf_t<typename M::Model, M::NX, M::NY>(models, a, s);
    });
}

}  // namespace llpf
