// k_simulate.hip — k_simulate (kernels/simulate.hpp): trajectories of a filter's model on the device (llpf_simulate / llpf_bank_simulate)
// One of the engine's device translation units (kernels.hip has the map).  The built-in models are instantiated here, by
// dispatch_builtin_model (kernels/dispatch.hpp); a run-time compiled model (a user snippet, the linear-Gaussian model above 4 states or
// outputs) gets its k_simulate from a program of its own (engine.hpp: JitProgram), compiled on the first simulation of that model and
// cached per model — the program of llpf_model_compile is left as it is.
#include "engine.hpp"
#include "jit_simulate.inc"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/reduce.hpp"
#include "kernels/models.hpp"
#include "kernels/simulate.hpp"
#include "kernels/dispatch.hpp"

template <class Model, int NX, int NY>
static hipError_t launch_simulate_t(const ModelD* models, int F, const SimArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.M + BLOCK - 1) / BLOCK), (unsigned)F, 1);
    hipLaunchKernelGGL((k_simulate<Model, NX, NY>), g, dim3(BLOCK), 0, s, models, a);
    return hipGetLastError();
}

// ---- run-time compiled models (engine.hpp: JitProgram, JitCache) ----
// by model id.  Kernel 0: k_simulate<UserModel, nx, ny>
static JitCache g_sim;

int simulate_prepare(int model_id, std::string& err) {
    if (model_id < LLPF_MODEL_USER_BASE) return 0;
    std::string snippet;
    int nx = 0, ny = 0;
    if (!jit_model_source(model_id, snippet, nx, ny)) { err = "unknown model id " + std::to_string(model_id); return -1; }
    return g_sim.prepare(std::to_string(model_id), [&]() {
        const std::string src = std::string(jit_prelude()) + "\nnamespace llpf {\n" + snippet + "\n" + LLPF_JIT_SIMULATE + "\n}  // namespace llpf\n";
        std::unique_ptr<JitProgram> p;
        // the options of the model's own program (kernels/jit.hpp) and of this unit (Makefile)
        jit_program_compile(src, "llpf_user_simulate.hip", {"llpf::k_simulate<llpf::UserModel, " + std::to_string(nx) + ", " + std::to_string(ny) + ">"},
                            {"-DLLPF_EXP_LDEXP=1"}, "hiprtc (k_simulate): ", p, err);
        return p;
    });
}

hipError_t launch_simulate(int model_id, int nx, int ny, const ModelD* models, int F, const SimArgs& a, hipStream_t s) {
    if (model_id >= LLPF_MODEL_USER_BASE) {
        hipFunction_t fn = nullptr;
        const hipError_t e = g_sim.function(std::to_string(model_id), 0, &fn);      // simulate_prepare compiles it first
        if (e != hipSuccess) return e;
        SimArgs aa = a;
        void* args[] = {&models, &aa};
        return hipModuleLaunchKernel(fn, (unsigned)((a.M + BLOCK - 1) / BLOCK), (unsigned)F, 1, BLOCK, 1, 1, 0, s, args, nullptr);
    }
    // (the linear-Gaussian model above 4 states or outputs comes with a run-time compiled model id: kernels/jit.hpp, jit_builtin_lg)
    return dispatch_builtin_model(model_id, nx, ny, [&](auto m) {
        using M = decltype(m);
        return launch_simulate_t<typename M::Model, M::NX, M::NY>(models, F, a, s);
    });
}

}  // namespace llpf
