// jit_sqekf_host.cpp — the run-time compile path of k_sqekf in libllpf_hip.so, driven without a device (tests/test_sqekf.py) the way
// tests/jit_programs_host.cpp drives the other units' paths.  hiprtc cross-compiles for gfx950 when no device is visible; nothing is
// loaded or launched.  The entry point is the engine's own (csrc/engine.hpp, namespace llpf), declared here so that the program needs
// neither the HIP headers nor a device compiler.
// Build: c++ -std=c++17 -I <root>/include jit_sqekf_host.cpp -L <package> -lllpf_hip -Wl,-rpath,<package> -o jit_sqekf_host
// Prints one line per check; the exit status is the number of failed checks.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "llpf.h"

namespace llpf {
int sqekf_prepare(int model_id, int nx, int ny, std::string& err);
}  // namespace llpf

// the built-in quad-tank as a snippet: its members, the two Jacobian ones among them, through a model id of its own
static const char* const QUADTANK_SNIPPET = R"SRC(
// tests/jit_sqekf_host.cpp
struct UserModel : QuadTank<4, 2> {};
)SRC";
// f(x) = x, g(x) = x_0^2 without the measurement's Jacobian: k_sqekf cannot be compiled for it
static const char* const SQUARE_NO_MEASUREMENT_JAC = R"SRC(
// tests/jit_sqekf_host.cpp
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const { fx[0] = x[0]; J[0] = 1.0; }
};
)SRC";

static int failed = 0;
static void check(bool ok, const char* what, const std::string& detail = "") {
    printf("%s %s%s%s\n", ok ? "ok  " : "FAIL", what, detail.empty() ? "" : ": ", detail.substr(0, 400).c_str());
    if (!ok) ++failed;
}
static bool starts_with(const std::string& s, const char* prefix) { return s.rfind(prefix, 0) == 0; }

int main() {
    using namespace llpf;
    const int LG = LLPF_MODEL_LINEAR_GAUSSIAN, QT = LLPF_MODEL_QUADTANK_RK4;
    std::string err;
    setenv("LLPF_JIT_COMPILE_ONLY", "1", 1);
    int32_t qt = -1, sq = -1;
    int rc = llpf_model_compile(QUADTANK_SNIPPET, 4, 2, &qt);
    check(rc == LLPF_OK && qt >= LLPF_MODEL_USER_BASE, "llpf_model_compile(quad-tank snippet)", rc == LLPF_OK ? "" : llpf_last_error());
    int32_t traits = 0;
    rc = llpf_model_traits(qt, &traits);
    check(rc == LLPF_OK && (traits & LLPF_TRAIT_DYNAMICS_JAC) && (traits & LLPF_TRAIT_MEASUREMENT_JAC), "the quad-tank snippet has both Jacobian members");
    // both programs compile, and the second call finds what the first one left
    for (int round = 0; round < 2; ++round) {
        const char* again = round ? " (again)" : "";
        err.clear(); check(sqekf_prepare(LG, 5, 1, err) == 0, (std::string("sqekf_prepare(LG, 5, 1)") + again).c_str(), err);
        err.clear(); check(sqekf_prepare(qt, 4, 2, err) == 0, (std::string("sqekf_prepare(quad-tank snippet, 4, 2)") + again).c_str(), err);
    }
    // the precompiled shapes need no program: 0, and nothing said
    err.clear();
    check(sqekf_prepare(LG, 4, 4, err) == 0 && sqekf_prepare(LG, 1, 1, err) == 0 && sqekf_prepare(QT, 4, 2, err) == 0 && err.empty(), "precompiled shapes", err);
    // an id nobody compiled: the message of the other units
    const int nobody = LLPF_MODEL_USER_BASE + 900;
    err.clear();
    check(sqekf_prepare(nobody, 2, 1, err) == -1 && err == "unknown model id " + std::to_string(nobody) + " at these dimensions", "sqekf_prepare(unknown id)", err);
    err.clear();
    check(sqekf_prepare(qt, 3, 2, err) == -1 && err == "unknown model id " + std::to_string(qt) + " at these dimensions", "sqekf_prepare(quad-tank snippet, other dimensions)", err);
    // a model the filter cannot be compiled for: the log comes back under the kernel's name
    rc = llpf_model_compile(SQUARE_NO_MEASUREMENT_JAC, 1, 1, &sq);
    check(rc == LLPF_OK && sq >= LLPF_MODEL_USER_BASE, "llpf_model_compile(x0^2 without measurement_jac)", rc == LLPF_OK ? "" : llpf_last_error());
    err.clear(); check(sqekf_prepare(sq, 1, 1, err) == -1 && starts_with(err, "hiprtc (k_sqekf): "), "sqekf_prepare(x0^2 without measurement_jac)", err);
    printf("%d failed\n", failed);
    return failed;
}
