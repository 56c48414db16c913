// k_ukf.hip — k_ukf, k_ukf_smooth (kernels/ukf.hpp): banks of unscented Kalman filters (llpf_ukf_bank_run, llpf_ukf_bank_smooth).
// One of the engine's device translation units: LinGauss<NX, NY> for NX, NY in 1..4 and QuadTank<4, 2> are instantiated here and nowhere
// else, for both kernels.  A run-time compiled model (a user snippet, a traced callable, the linear-Gaussian model above 4 states) gets
// its k_ukf from a hiprtc program of its own, compiled on the first bank of that model and cached per model — the program of
// llpf_model_compile is left as it is — and its k_ukf_smooth, with the posterior-storing k_ukf<..., true> of the smoother's forward pass,
// from another one, compiled on the first smooth of that model and cached in an entry of its own: a bank that never smooths compiles what
// it always did.
#include <hip/hiprtc.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "shared/llpf_ukf.h"
#include "jit_ukf.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/ukf.hpp"
#include "kernels/jit_bank.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_ukf_t(const ModelD* models, const UkfArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1);
    if (a.post)
        hipLaunchKernelGGL((k_ukf<Model, NX, NY, true>), g, dim3(KF_BLOCK), 0, s, models, a);
    else
        hipLaunchKernelGGL((k_ukf<Model, NX, NY, false>), g, dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
template <class Model, int NX>
static hipError_t launch_ukf_smooth_t(const ModelD* models, const UkfSmoothArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1);
    hipLaunchKernelGGL((k_ukf_smooth<Model, NX>), g, dim3(KF_BLOCK), 0, s, models, a);
    return hipGetLastError();
}
template <int NX>
static hipError_t launch_ukf_lg(int ny, const ModelD* models, const UkfArgs& a, hipStream_t s) {
    switch (ny) {
        case 1: return launch_ukf_t<LinGauss<NX, 1>, NX, 1>(models, a, s);
        case 2: return launch_ukf_t<LinGauss<NX, 2>, NX, 2>(models, a, s);
        case 3: return launch_ukf_t<LinGauss<NX, 3>, NX, 3>(models, a, s);
        case 4: return launch_ukf_t<LinGauss<NX, 4>, NX, 4>(models, a, s);
        default: return hipErrorInvalidValue;
    }
}
template <int NX>
static hipError_t launch_ukf_smooth_lg(int ny, const ModelD* models, const UkfSmoothArgs& a, hipStream_t s) {
    switch (ny) {
        case 1: return launch_ukf_smooth_t<LinGauss<NX, 1>, NX>(models, a, s);
        case 2: return launch_ukf_smooth_t<LinGauss<NX, 2>, NX>(models, a, s);
        case 3: return launch_ukf_smooth_t<LinGauss<NX, 3>, NX>(models, a, s);
        case 4: return launch_ukf_smooth_t<LinGauss<NX, 4>, NX>(models, a, s);
        default: return hipErrorInvalidValue;
    }
}

// ---- run-time compiled models (kernels/jit_bank.hpp) ----
// by ukf_key: the forward and the backward kernel are entries of their own.  Kernel 0: k_ukf<UserModel, nx, ny> of a forward entry,
// k_ukf_smooth<UserModel, nx> of a smoother's; kernel 1 of a smoother's entry: k_ukf<UserModel, nx, ny, true>, its forward pass
static std::mutex g_ukf_mutex;
static std::map<std::string, std::unique_ptr<JitBankKernels>> g_ukf;

static bool ukf_builtin(int model_id, int nx, int ny) {
    return (model_id == LLPF_MODEL_LINEAR_GAUSSIAN && nx <= 4 && ny <= 4) || model_id == LLPF_MODEL_QUADTANK_RK4;
}
static std::string ukf_key(int model_id, int nx, int ny, bool smooth) {
    return std::to_string(model_id) + ":" + std::to_string(nx) + ":" + std::to_string(ny) + (smooth ? ":smooth" : "");
}

// compiles k_ukf (smooth = false), or k_ukf_smooth and the posterior-storing k_ukf<..., true> (smooth = true), of a run-time compiled
// model unless its entry exists
static int ukf_compile(int model_id, int nx, int ny, bool smooth, std::string& err) {
    if (ukf_builtin(model_id, nx, ny)) return 0;
    const std::string key = ukf_key(model_id, nx, ny, smooth);
    {
        std::lock_guard<std::mutex> lk(g_ukf_mutex);
        if (g_ukf.count(key)) return 0;
    }
    std::string snippet;
    if (!jit_bank_snippet(model_id, nx, ny, snippet)) { err = "unknown model id " + std::to_string(model_id) + " at these dimensions"; return -1; }
    std::vector<std::string> exprs;
    if (smooth) {
        exprs.push_back("llpf::k_ukf_smooth<llpf::UserModel, " + std::to_string(nx) + ">");
        exprs.push_back("llpf::k_ukf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ", true>");
    } else {
        exprs.push_back("llpf::k_ukf<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ">");
    }
    std::unique_ptr<JitBankKernels> jk;
    if (jit_bank_compile(LLPF_JIT_UKF_SHARED, snippet, LLPF_JIT_UKF, "llpf_user_ukf.hip", exprs, smooth ? "k_ukf_smooth" : "k_ukf", jk, err) != 0) return -1;
    std::lock_guard<std::mutex> lk(g_ukf_mutex);
    if (!g_ukf.count(key)) g_ukf[key] = std::move(jk);      // another thread may have compiled it meanwhile: the first one stays
    return 0;
}

int ukf_prepare(int model_id, int nx, int ny, std::string& err) { return ukf_compile(model_id, nx, ny, false, err); }
int ukf_smooth_prepare(int model_id, int nx, int ny, std::string& err) { return ukf_compile(model_id, nx, ny, true, err); }

// this device's handle of the compiled kernel (loaded on first use); post: the smoother's forward kernel k_ukf<..., true>
static hipError_t ukf_function(int model_id, int nx, int ny, bool smooth, bool post, hipFunction_t* fn) {
    std::lock_guard<std::mutex> lk(g_ukf_mutex);
    auto it = g_ukf.find(ukf_key(model_id, nx, ny, smooth));
    if (it == g_ukf.end()) return hipErrorInvalidValue;      // ukf_prepare / ukf_smooth_prepare compiles it first
    return jit_bank_function(*it->second, post ? 1 : 0, fn);
}

hipError_t launch_ukf(int model_id, int nx, int ny, const ModelD* models, const UkfArgs& a, hipStream_t s) {
    if (!ukf_builtin(model_id, nx, ny)) {
        hipFunction_t fn = nullptr;
        const hipError_t e = a.post ? ukf_function(model_id, nx, ny, true, true, &fn) : ukf_function(model_id, nx, ny, false, false, &fn);
        if (e != hipSuccess) return e;
        UkfArgs aa = a;
        void* args[] = {&models, &aa};
        return hipModuleLaunchKernel(fn, (unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1, KF_BLOCK, 1, 1, 0, s, args, nullptr);
    }
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2) return hipErrorInvalidValue;
        return launch_ukf_t<QuadTank<4, 2>, 4, 2>(models, a, s);
    }
    switch (nx) {
        case 1: return launch_ukf_lg<1>(ny, models, a, s);
        case 2: return launch_ukf_lg<2>(ny, models, a, s);
        case 3: return launch_ukf_lg<3>(ny, models, a, s);
        case 4: return launch_ukf_lg<4>(ny, models, a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ukf_smooth(int model_id, int nx, int ny, const ModelD* models, const UkfSmoothArgs& a, hipStream_t s) {
    if (!ukf_builtin(model_id, nx, ny)) {
        hipFunction_t fn = nullptr;
        const hipError_t e = ukf_function(model_id, nx, ny, true, false, &fn);
        if (e != hipSuccess) return e;
        UkfSmoothArgs aa = a;
        void* args[] = {&models, &aa};
        return hipModuleLaunchKernel(fn, (unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1, KF_BLOCK, 1, 1, 0, s, args, nullptr);
    }
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2) return hipErrorInvalidValue;
        return launch_ukf_smooth_t<QuadTank<4, 2>, 4>(models, a, s);
    }
    switch (nx) {
        case 1: return launch_ukf_smooth_lg<1>(ny, models, a, s);
        case 2: return launch_ukf_smooth_lg<2>(ny, models, a, s);
        case 3: return launch_ukf_smooth_lg<3>(ny, models, a, s);
        case 4: return launch_ukf_smooth_lg<4>(ny, models, a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace llpf
