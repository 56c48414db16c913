// k_simulate.hip — k_simulate (kernels/simulate.hpp): trajectories of a filter's model on the device (llpf_simulate / llpf_bank_simulate)
// One of the engine's device translation units (kernels.hip has the map).  The built-in models are instantiated here; a run-time compiled
// model (a user snippet, the linear-Gaussian model above 4 states or outputs) gets its k_simulate from a hiprtc program of its own, compiled
// on the first simulation of that model and cached per model and device — the program of llpf_model_compile is left as it is.
#include <hip/hiprtc.h>

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "jit_simulate.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/simulate.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_simulate_t(const ModelD* models, int F, const SimArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.M + BLOCK - 1) / BLOCK), (unsigned)F, 1);
    hipLaunchKernelGGL((k_simulate<Model, NX, NY>), g, dim3(BLOCK), 0, s, models, a);
    return hipGetLastError();
}
template <int NX>
static hipError_t launch_simulate_lg(int ny, const ModelD* models, int F, const SimArgs& a, hipStream_t s) {
    switch (ny) {
        case 1: return launch_simulate_t<LinGauss<NX, 1>, NX, 1>(models, F, a, s);
        case 2: return launch_simulate_t<LinGauss<NX, 2>, NX, 2>(models, F, a, s);
        case 3: return launch_simulate_t<LinGauss<NX, 3>, NX, 3>(models, F, a, s);
        case 4: return launch_simulate_t<LinGauss<NX, 4>, NX, 4>(models, F, a, s);
        default: return hipErrorInvalidValue;
    }
}

// ---- run-time compiled models ----
struct JitSim {
    std::vector<char> code;
    std::string name;                          // lowered name of k_simulate<UserModel, nx, ny>
    struct PerDevice { hipModule_t mod = nullptr; hipFunction_t fn = nullptr; };
    std::vector<PerDevice> dev;                // indexed by device ordinal, loaded on first use
};
static std::mutex g_sim_mutex;
static std::map<int, std::unique_ptr<JitSim>> g_sim;      // by model id

static int jit_sim_compile(int model_id, std::string& err) {
    std::string snippet;
    int nx = 0, ny = 0;
    if (!jit_model_source(model_id, snippet, nx, ny)) { err = "unknown model id " + std::to_string(model_id); return -1; }
    {
        std::lock_guard<std::mutex> lk(g_sim_mutex);
        if (g_sim.count(model_id)) return 0;
    }
    std::string src(jit_prelude());
    src += "\nnamespace llpf {\n";
    src += snippet;
    src += "\n";
    src += LLPF_JIT_SIMULATE;
    src += "\n}  // namespace llpf\n";
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), "llpf_user_simulate.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) { err = "hiprtcCreateProgram failed"; return -1; }
    const std::string expr = "llpf::k_simulate<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ">";
    hiprtcAddNameExpression(prog, expr.c_str());
    int devid = 0;
    hipDeviceProp_t prop;
    std::string arch = "gfx950";
    if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.gcnArchName[0]) arch = prop.gcnArchName;
    const std::string archopt = "--offload-arch=" + arch;
    // the options of the model's own program (kernels/jit.hpp) and of this unit (Makefile): -ffp-contract=off, the same bits
    const char* opts[] = {archopt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value", "-DLLPF_EXP_LDEXP=1"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        err = std::string("hiprtc (k_simulate): ") + hiprtcGetErrorString(rc) + "\n" + log;
        hiprtcDestroyProgram(&prog);
        return -1;
    }
    std::unique_ptr<JitSim> js(new JitSim());
    size_t sz = 0;
    hiprtcGetCodeSize(prog, &sz);
    js->code.resize(sz);
    hiprtcGetCode(prog, js->code.data());
    const char* low = nullptr;
    if (hiprtcGetLoweredName(prog, expr.c_str(), &low) != HIPRTC_SUCCESS || !low) { err = "hiprtcGetLoweredName failed for " + expr; hiprtcDestroyProgram(&prog); return -1; }
    js->name = low;
    hiprtcDestroyProgram(&prog);
    std::lock_guard<std::mutex> lk(g_sim_mutex);
    if (!g_sim.count(model_id)) g_sim[model_id] = std::move(js);      // another thread may have compiled it meanwhile: the first one stays
    return 0;
}

int simulate_prepare(int model_id, std::string& err) {
    if (model_id < LLPF_MODEL_USER_BASE) return 0;
    return jit_sim_compile(model_id, err);
}

hipError_t launch_simulate(int model_id, int nx, int ny, const ModelD* models, int F, const SimArgs& a, hipStream_t s) {
    if (model_id >= LLPF_MODEL_USER_BASE) {
        int devid = 0;
        hipError_t e = hipGetDevice(&devid);
        if (e != hipSuccess) return e;
        hipFunction_t fn = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_sim_mutex);
            auto it = g_sim.find(model_id);
            if (it == g_sim.end()) return hipErrorInvalidValue;      // simulate_prepare compiles it first
            JitSim& js = *it->second;
            if ((int)js.dev.size() <= devid) js.dev.resize((size_t)devid + 1);
            JitSim::PerDevice& pd = js.dev[(size_t)devid];
            if (!pd.mod && (e = hipModuleLoadData(&pd.mod, js.code.data())) != hipSuccess) return e;
            if (!pd.fn && (e = hipModuleGetFunction(&pd.fn, pd.mod, js.name.c_str())) != hipSuccess) return e;
            fn = pd.fn;
        }
        SimArgs aa = a;
        void* args[] = {&models, &aa};
        return hipModuleLaunchKernel(fn, (unsigned)((a.M + BLOCK - 1) / BLOCK), (unsigned)F, 1, BLOCK, 1, 1, 0, s, args, nullptr);
    }
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2) return hipErrorInvalidValue;
        return launch_simulate_t<QuadTank<4, 2>, 4, 2>(models, F, a, s);
    }
    if (model_id != LLPF_MODEL_LINEAR_GAUSSIAN) return hipErrorInvalidValue;
    switch (nx) {
        case 1: return launch_simulate_lg<1>(ny, models, F, a, s);
        case 2: return launch_simulate_lg<2>(ny, models, F, a, s);
        case 3: return launch_simulate_lg<3>(ny, models, F, a, s);
        case 4: return launch_simulate_lg<4>(ny, models, F, a, s);
        default: return hipErrorInvalidValue;        // above 4: a run-time compiled model id (kernels/jit.hpp: jit_builtin_lg)
    }
}

}  // namespace llpf
