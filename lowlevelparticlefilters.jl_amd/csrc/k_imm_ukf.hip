// k_imm_ukf.hip — k_imm_ukf (kernels/imm_ukf.hpp: ImmUkfMode in the step frame imm_chunk of kernels/imm.hpp): banks of
// interacting-multiple-model filters over unscented Kalman filters of one model type (llpf_imm_bank_run_at on an unscented bank).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2>, each at G = 1, 2 and 4, are
// instantiated here and nowhere else, by dispatch_builtin_model (kernels/dispatch.hpp).  A run-time compiled model (a user snippet or a
// traced callable, with or without Jacobian members, the linear-Gaussian model above 4 states) gets its k_imm_ukf from a program of its
// own (engine.hpp: JitProgram; kernels/jit_bank.hpp), compiled on the first unscented IMM bank of that model and group size and cached
// per (model id, nx, ny, G): the programs and cache entries of the other units are left as they are.
#include "engine.hpp"
#include "shared/llpf_ukf.h"
#include "shared/llpf_imm.h"
#include "jit_imm_ukf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/imm_args.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/ukf.hpp"
#include "kernels/imm.hpp"
#include "kernels/imm_ukf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"

// one lane per (filter, mode): F * G lanes
template <class Model, int NX, int NY, int G>
static hipError_t launch_imm_ukf_t(const ModelD* models, const ImmUkfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_imm_ukf<Model, NX, NY, G>), kf_grid(a.F * G), dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}

// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// One entry per group size.  Kernel 0: k_imm_ukf<UserModel, nx, ny, G>
static JitCache g_imm_ukf;

static std::string imm_ukf_key(int model_id, int nx, int ny, int g) { return jit_bank_key(model_id, nx, ny, (":g" + std::to_string(g)).c_str()); }

int imm_ukf_prepare(int model_id, int nx, int ny, int g, std::string& err) {
    if (jit_bank_builtin(model_id, nx, ny)) return 0;
    return g_imm_ukf.prepare(imm_ukf_key(model_id, nx, ny, g), [&]() {
        const std::string expr = "llpf::k_imm_ukf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ", " + std::to_string(g) + ">";
        return jit_bank_build(model_id, nx, ny, LLPF_JIT_IMM_UKF_SHARED, LLPF_JIT_IMM_UKF, "llpf_user_imm_ukf.hip", {expr}, "hiprtc (k_imm_ukf): ", err);
    });
}

// g: the lanes per filter, 1, 2 or 4 (imm_group)
hipError_t launch_imm_ukf(int model_id, int nx, int ny, int g, const ModelD* models, const ImmUkfArgs& a, hipStream_t s) {
    if (g != 1 && g != 2 && g != 4) return hipErrorInvalidValue;
    if (!jit_bank_builtin(model_id, nx, ny)) return jit_bank_launch(g_imm_ukf, imm_ukf_key(model_id, nx, ny, g), 0, models, a, a.F * g, s);
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using T = decltype(m);
        using Mo = typename T::Model;
        return g == 1 ? launch_imm_ukf_t<Mo, T::NX, T::NY, 1>(models, a, s)
             : g == 2 ? launch_imm_ukf_t<Mo, T::NX, T::NY, 2>(models, a, s)
                      : launch_imm_ukf_t<Mo, T::NX, T::NY, 4>(models, a, s);
    });
}

}  // namespace llpf
