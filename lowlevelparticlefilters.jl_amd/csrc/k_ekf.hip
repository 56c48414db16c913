// k_ekf.hip — k_ekf (kernels/ekf.hpp): banks of extended and of iterated extended Kalman filters (llpf_ekf_bank_run).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here and nowhere
// else, for both kernels.  A run-time compiled model (a user snippet or a traced callable with dynamics_jac and measurement_jac, the
// linear-Gaussian model above 4 states) gets its k_ekf from a hiprtc program of its own, compiled on the first bank of that model and
// cached per (model id, nx, ny) — the programs of llpf_model_compile, k_simulate and k_ukf are left as they are — and its iterated
// kernel k_ekf<..., IekfArgs> from another one, compiled on the first iterated use of that model and cached in an entry of its own: a
// bank that never iterates compiles what it always did.
#include <hip/hiprtc.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "shared/llpf_ekf.h"
#include "jit_ekf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/ekf.hpp"
#include "kernels/jit_bank.hpp"

// ia: null for the plain kernel, or the arguments of the iterated one, k_ekf<..., IekfArgs> (its EkfArgs part is `a`)
template <class Model, int NX, int NY>
static hipError_t launch_ekf_t(const ModelD* models, const EkfArgs& a, const IekfArgs* ia, hipStream_t s) {
    const dim3 g((unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1);
    if (ia)
        hipLaunchKernelGGL((k_ekf<Model, NX, NY, IekfArgs>), g, dim3(KF_BLOCK), 0, s, models, *ia);
    else
        hipLaunchKernelGGL((k_ekf<Model, NX, NY>), g, dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
template <int NX>
static hipError_t launch_ekf_lg(int ny, const ModelD* models, const EkfArgs& a, const IekfArgs* ia, hipStream_t s) {
    switch (ny) {
        case 1: return launch_ekf_t<LinGauss<NX, 1>, NX, 1>(models, a, ia, s);
        case 2: return launch_ekf_t<LinGauss<NX, 2>, NX, 2>(models, a, ia, s);
        case 3: return launch_ekf_t<LinGauss<NX, 3>, NX, 3>(models, a, ia, s);
        case 4: return launch_ekf_t<LinGauss<NX, 4>, NX, 4>(models, a, ia, s);
        default: return hipErrorInvalidValue;
    }
}

// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// by ekf_key: the plain and the iterated kernel are entries of their own.  Kernel 0: k_ekf<UserModel, nx, ny>, or
// k_ekf<UserModel, nx, ny, IekfArgs>
static std::mutex g_ekf_mutex;
static std::map<std::string, std::unique_ptr<JitBankKernels>> g_ekf;

static bool ekf_builtin(int model_id, int nx, int ny) {
    return (model_id == LLPF_MODEL_LINEAR_GAUSSIAN && nx <= 4 && ny <= 4) || model_id == LLPF_MODEL_QUADTANK_RK4;
}
static std::string ekf_key(int model_id, int nx, int ny, bool iterated) {
    return std::to_string(model_id) + ":" + std::to_string(nx) + ":" + std::to_string(ny) + (iterated ? ":iterated" : "");
}

// compiles k_ekf (iterated = false) or k_ekf<..., IekfArgs> (iterated = true) of a run-time compiled model unless its entry exists
static int ekf_compile(int model_id, int nx, int ny, bool iterated, std::string& err) {
    if (ekf_builtin(model_id, nx, ny)) return 0;
    const std::string key = ekf_key(model_id, nx, ny, iterated);
    {
        std::lock_guard<std::mutex> lk(g_ekf_mutex);
        if (g_ekf.count(key)) return 0;
    }
    std::string snippet;
    if (!jit_bank_snippet(model_id, nx, ny, snippet)) { err = "unknown model id " + std::to_string(model_id) + " at these dimensions"; return -1; }
    const char* kernel = iterated ? "k_ekf, iterated" : "k_ekf";
    const std::vector<std::string> exprs = {"llpf::k_ekf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + (iterated ? ", llpf::IekfArgs>" : ">")};
    std::unique_ptr<JitBankKernels> jk;
    if (jit_bank_compile(LLPF_JIT_EKF_SHARED, snippet, LLPF_JIT_EKF, "llpf_user_ekf.hip", exprs, kernel, jk, err) != 0) return -1;
    std::lock_guard<std::mutex> lk(g_ekf_mutex);
    if (!g_ekf.count(key)) g_ekf[key] = std::move(jk);      // another thread may have compiled it meanwhile: the first one stays
    return 0;
}

int ekf_prepare(int model_id, int nx, int ny, std::string& err) { return ekf_compile(model_id, nx, ny, false, err); }
int iekf_prepare(int model_id, int nx, int ny, std::string& err) { return ekf_compile(model_id, nx, ny, true, err); }

// this device's handle of the compiled kernel (loaded on first use)
static hipError_t ekf_function(int model_id, int nx, int ny, bool iterated, hipFunction_t* fn) {
    std::lock_guard<std::mutex> lk(g_ekf_mutex);
    auto it = g_ekf.find(ekf_key(model_id, nx, ny, iterated));
    if (it == g_ekf.end()) return hipErrorInvalidValue;      // ekf_prepare / iekf_prepare compiles it first
    return jit_bank_function(*it->second, 0, fn);
}

static hipError_t launch_ekf_any(int model_id, int nx, int ny, const ModelD* models, const EkfArgs& a, const IekfArgs* ia, hipStream_t s) {
    if (!ekf_builtin(model_id, nx, ny)) {
        hipFunction_t fn = nullptr;
        const hipError_t e = ekf_function(model_id, nx, ny, ia != nullptr, &fn);
        if (e != hipSuccess) return e;
        EkfArgs aa = a;
        IekfArgs iaa = ia ? *ia : IekfArgs{};
        void* args[] = {&models, ia ? (void*)&iaa : (void*)&aa};
        return hipModuleLaunchKernel(fn, (unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1, KF_BLOCK, 1, 1, 0, s, args, nullptr);
    }
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2) return hipErrorInvalidValue;
        return launch_ekf_t<QuadTank<4, 2>, 4, 2>(models, a, ia, s);
    }
    switch (nx) {
        case 1: return launch_ekf_lg<1>(ny, models, a, ia, s);
        case 2: return launch_ekf_lg<2>(ny, models, a, ia, s);
        case 3: return launch_ekf_lg<3>(ny, models, a, ia, s);
        case 4: return launch_ekf_lg<4>(ny, models, a, ia, s);
        default: return hipErrorInvalidValue;
    }
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
