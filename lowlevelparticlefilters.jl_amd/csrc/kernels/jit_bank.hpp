// kernels/jit_bank.hpp — what the run-time programs of the model-driven Kalman banks share (host side; part of k_ukf.hip and k_ekf.hip,
// namespace llpf): the hiprtc compile of one program around a model's snippet, its lowered kernel names, and the per-device module.
// ------------------------------------------------------------------------------------------------
// A program is the prelude, the bank's shared headers at file scope, then inside namespace llpf the snippet and the bank's kernel text.
// The options are those of the banks' own translation units (Makefile): -ffp-contract=off, the same bits.  Each unit keeps its own cache
// of these entries under its own mutex; the functions here take no lock.
struct JitBankKernels {
    std::vector<char> code;
    std::vector<std::string> names;            // lowered names, in the order of the name expressions given to the compile
    struct PerDevice { hipModule_t mod = nullptr; std::vector<hipFunction_t> fn; };
    std::vector<PerDevice> dev;                // indexed by device ordinal, loaded on first use
};

// the snippet of a bank's model: a user model's own source, or LinGauss<nx, ny> above the precompiled dimensions
static bool jit_bank_snippet(int model_id, int nx, int ny, std::string& snippet) {
    if (model_id == LLPF_MODEL_LINEAR_GAUSSIAN) {
        snippet = "struct UserModel : LinGauss<" + std::to_string(nx) + ", " + std::to_string(ny) + "> {};\n";
        return true;
    }
    int sx = 0, sy = 0;
    return jit_model_source(model_id, snippet, sx, sy) && sx == nx && sy == ny;
}

// compiles the program and resolves `exprs` (kernel name expressions); `what` names the kernel in an error.  0, or -1 with `err` set
static int jit_bank_compile(const char* shared_text, const std::string& snippet, const char* kernel_text, const char* file,
                            const std::vector<std::string>& exprs, const char* what, std::unique_ptr<JitBankKernels>& out, std::string& err) {
    std::string src(jit_prelude());
    src += "\n";
    src += shared_text;
    src += "\nnamespace llpf {\n";
    src += snippet;
    src += "\n";
    src += kernel_text;
    src += "\n}  // namespace llpf\n";
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), file, 0, nullptr, nullptr) != HIPRTC_SUCCESS) { err = "hiprtcCreateProgram failed"; return -1; }
    for (const std::string& e : exprs) hiprtcAddNameExpression(prog, e.c_str());
    int devid = 0;
    hipDeviceProp_t prop;
    std::string arch = "gfx950";
    if (hipGetDevice(&devid) == hipSuccess && hipGetDeviceProperties(&prop, devid) == hipSuccess && prop.gcnArchName[0]) arch = prop.gcnArchName;
    const std::string archopt = "--offload-arch=" + arch;
    const char* opts[] = {archopt.c_str(), "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-value"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        err = std::string("hiprtc (") + what + "): " + hiprtcGetErrorString(rc) + "\n" + log;
        hiprtcDestroyProgram(&prog);
        return -1;
    }
    std::unique_ptr<JitBankKernels> jk(new JitBankKernels());
    size_t sz = 0;
    hiprtcGetCodeSize(prog, &sz);
    jk->code.resize(sz);
    hiprtcGetCode(prog, jk->code.data());
    for (const std::string& e : exprs) {
        const char* low = nullptr;
        if (hiprtcGetLoweredName(prog, e.c_str(), &low) != HIPRTC_SUCCESS || !low) { err = "hiprtcGetLoweredName failed for " + e; hiprtcDestroyProgram(&prog); return -1; }
        jk->names.push_back(low);
    }
    hiprtcDestroyProgram(&prog);
    out = std::move(jk);
    return 0;
}

// the current device's handle of kernel `which` of the program (module and function loaded on first use); the caller holds its lock
static hipError_t jit_bank_function(JitBankKernels& jk, int which, hipFunction_t* fn) {
    int devid = 0;
    hipError_t e = hipGetDevice(&devid);
    if (e != hipSuccess) return e;
    if ((int)jk.dev.size() <= devid) jk.dev.resize((size_t)devid + 1);
    JitBankKernels::PerDevice& pd = jk.dev[(size_t)devid];
    if (!pd.mod && (e = hipModuleLoadData(&pd.mod, jk.code.data())) != hipSuccess) return e;
    if (pd.fn.size() < jk.names.size()) pd.fn.resize(jk.names.size(), nullptr);
    if (!pd.fn[(size_t)which] && (e = hipModuleGetFunction(&pd.fn[(size_t)which], pd.mod, jk.names[(size_t)which].c_str())) != hipSuccess) return e;
    *fn = pd.fn[(size_t)which];
    return hipSuccess;
}
