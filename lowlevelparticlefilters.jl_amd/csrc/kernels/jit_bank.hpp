// kernels/jit_bank.hpp — what the run-time programs of the model-driven Kalman banks share (host side; part of k_ukf.hip and k_ekf.hip,
// namespace llpf): which models have precompiled kernels, the key of a cache entry, and the source of one program around a model's snippet.
// ------------------------------------------------------------------------------------------------
// A program is the prelude, the bank's shared headers at file scope, then inside namespace llpf the snippet and the bank's kernel text.
// It is compiled by jit_program_compile without extra options and kept in the unit's own JitCache (engine.hpp).
static bool jit_bank_builtin(int model_id, int nx, int ny) {
    return (model_id == LLPF_MODEL_LINEAR_GAUSSIAN && nx <= 4 && ny <= 4) || model_id == LLPF_MODEL_QUADTANK_RK4;
}
// `variant`: "" or the suffix of a second entry of the same model (":smooth", ":iterated")
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
