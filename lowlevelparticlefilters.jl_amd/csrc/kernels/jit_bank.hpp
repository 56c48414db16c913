// kernels/jit_bank.hpp — what the launchers of the one-thread-per-filter banks share (host side; part of k_kalman.hip, k_ukf.hip,
// k_ekf.hip and — one lane per (filter, mode) — k_imm_ekf.hip and k_imm_ukf.hip, namespace llpf, after kernels/kf_store.hpp): the grid of a bank and, for the model-driven banks, which models have precompiled
// kernels, the key of a cache entry, the source of one program around a model's snippet, and the launch of a kernel of such a program.
// ------------------------------------------------------------------------------------------------
// one thread per filter, KF_BLOCK of them per workgroup
static dim3 kf_grid(int64_t F) { return dim3((unsigned)((F + KF_BLOCK - 1) / KF_BLOCK), 1, 1); }

// A program is the prelude, the bank's shared headers at file scope, then inside namespace llpf the snippet and the bank's kernel text.
// It is compiled by jit_program_compile without extra options and kept in the unit's own JitCache (engine.hpp).
static bool jit_bank_builtin(int model_id, int nx, int ny) {
    return (model_id == LLPF_MODEL_LINEAR_GAUSSIAN && nx <= 4 && ny <= 4) || model_id == LLPF_MODEL_QUADTANK_RK4;
}
// `variant`: "" or the suffix of a second entry of the same model (":smooth", ":iterated", k_imm_ekf's and k_imm_ukf's ":g<lanes per filter>")
static std::string jit_bank_key(int model_id, int nx, int ny, const char* variant) {
    return std::to_string(model_id) + ":" + std::to_string(nx) + ":" + std::to_string(ny) + variant;
}

// the program of a bank's model — a user model's own snippet, or LinGauss<nx, ny> above the precompiled dimensions — with the kernels
// `exprs`; `what` is the prefix of a compile error.  Null with `err` set when the model is unknown or does not compile
static std::unique_ptr<JitProgram> jit_bank_build(int model_id, int nx, int ny, const char* shared_text, const char* kernel_text, const char* file,
                                                  const std::vector<std::string>& exprs, const char* what, std::string& err) {
    std::string snippet;
    int sx = 0, sy = 0;
    if (model_id == LLPF_MODEL_LINEAR_GAUSSIAN) snippet = "struct UserModel : LinGauss<" + std::to_string(nx) + ", " + std::to_string(ny) + "> {};\n";
    else if (!jit_model_source(model_id, snippet, sx, sy) || sx != nx || sy != ny) { err = "unknown model id " + std::to_string(model_id) + " at these dimensions"; return nullptr; }
    const std::string src = std::string(jit_prelude()) + "\n" + shared_text + "\nnamespace llpf {\n" + snippet + "\n" + kernel_text + "\n}  // namespace llpf\n";
    std::unique_ptr<JitProgram> p;
    jit_program_compile(src, file, exprs, {}, what, p, err);
    return p;
}

// launches kernel `which` of the entry `key` of the unit's cache (its prepare compiled it) as k(models, args) over F filters (threads)
template <class Args>
static hipError_t jit_bank_launch(JitCache& cache, const std::string& key, int which, const ModelD* models, Args args, int64_t F, hipStream_t s) {
    hipFunction_t fn = nullptr;
    const hipError_t e = cache.function(key, which, &fn);
    if (e != hipSuccess) return e;
    void* params[] = {&models, &args};
    return hipModuleLaunchKernel(fn, kf_grid(F).x, 1, 1, KF_BLOCK, 1, 1, 0, s, params, nullptr);
}
