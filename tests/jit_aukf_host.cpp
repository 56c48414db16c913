// jit_aukf_host.cpp — the run-time compile path of k_aukf in libllpf_hip.so, driven without a device (tests/test_aukf.py) the way
// tests/jit_sqekf_host.cpp drives k_sqekf's.  hiprtc cross-compiles for gfx950 when no device is visible; nothing is loaded or launched.
// The entry point is the engine's own (csrc/engine.hpp, namespace llpf), declared here so that the program needs neither the HIP headers
// nor a device compiler.
// Build: c++ -std=c++17 -I <root>/include jit_aukf_host.cpp -L <package> -lllpf_hip -Wl,-rpath,<package> -o jit_aukf_host
// Prints one line per check; the exit status is the number of failed checks.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "llpf.h"

namespace llpf {
int aukf_prepare(int model_id, int nx, int ny, std::string& err);
}  // namespace llpf

// x' = a x (1 + w) + w^2, g(x) = x^2: a model with dynamics_w
static const char* const WITH_MEMBER = R"SRC(
// tests/jit_aukf_host.cpp
struct UserModel {
    static constexpr bool RB = false;
    double a;
    DEV void prepare(const ModelD* m, const double* u, double t) { a = m->qt[0]; }
    DEV void dynamics_w(const double* x, const double* w, double* out) const { out[0] = a * x[0] * (1.0 + w[0]) + w[0] * w[0]; }
    DEV void dynamics(const double* x, double* out) const { out[0] = a * x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
};
)SRC";
// the same model without the member: the additive path
static const char* const WITHOUT_MEMBER = R"SRC(
// tests/jit_aukf_host.cpp
struct UserModel {
    static constexpr bool RB = false;
    double a;
    DEV void prepare(const ModelD* m, const double* u, double t) { a = m->qt[0]; }
    DEV void dynamics(const double* x, double* out) const { out[0] = a * x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
};
)SRC";
// a member with another signature: k_aukf cannot be compiled for it
static const char* const WRONG_MEMBER = R"SRC(
// tests/jit_aukf_host.cpp
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics_w(const double* x, double* out) const { out[0] = x[0]; }
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
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
    int32_t with = -1, without = -1, wrong = -1, traits = 0;
    int rc = llpf_model_compile(WITH_MEMBER, 1, 1, &with);
    check(rc == LLPF_OK && with >= LLPF_MODEL_USER_BASE, "llpf_model_compile(with dynamics_w)", rc == LLPF_OK ? "" : llpf_last_error());
    rc = llpf_model_traits(with, &traits);
    check(rc == LLPF_OK && traits == LLPF_TRAIT_DYNAMICS_W, "the snippet with the member reports LLPF_TRAIT_DYNAMICS_W alone");
    rc = llpf_model_compile(WITHOUT_MEMBER, 1, 1, &without);
    check(rc == LLPF_OK && without >= LLPF_MODEL_USER_BASE, "llpf_model_compile(without dynamics_w)", rc == LLPF_OK ? "" : llpf_last_error());
    rc = llpf_model_traits(without, &traits);
    check(rc == LLPF_OK && traits == 0, "the snippet without the member reports no trait");
    // the three programs compile — (LG, 8, 4) is the 132 KiB array of mapped points in LDS — and the second call finds what the first left
    for (int round = 0; round < 2; ++round) {
        const char* again = round ? " (again)" : "";
        err.clear(); check(aukf_prepare(with, 1, 1, err) == 0, (std::string("aukf_prepare(with dynamics_w, 1, 1)") + again).c_str(), err);
        err.clear(); check(aukf_prepare(without, 1, 1, err) == 0, (std::string("aukf_prepare(without dynamics_w, 1, 1)") + again).c_str(), err);
        err.clear(); check(aukf_prepare(LG, 8, 4, err) == 0, (std::string("aukf_prepare(LG, 8, 4)") + again).c_str(), err);
    }
    // the precompiled shapes need no program: 0, and nothing said
    err.clear();
    check(aukf_prepare(LG, 4, 4, err) == 0 && aukf_prepare(LG, 1, 1, err) == 0 && aukf_prepare(QT, 4, 2, err) == 0 && err.empty(), "precompiled shapes", err);
    // an id nobody compiled: the message of the other units
    const int nobody = LLPF_MODEL_USER_BASE + 900;
    err.clear();
    check(aukf_prepare(nobody, 2, 1, err) == -1 && err == "unknown model id " + std::to_string(nobody) + " at these dimensions", "aukf_prepare(unknown id)", err);
    // a member the kernel cannot call: the log comes back under the kernel's name
    rc = llpf_model_compile(WRONG_MEMBER, 1, 1, &wrong);
    check(rc == LLPF_OK && wrong >= LLPF_MODEL_USER_BASE, "llpf_model_compile(dynamics_w of another signature)", rc == LLPF_OK ? "" : llpf_last_error());
    err.clear(); check(aukf_prepare(wrong, 1, 1, err) == -1 && starts_with(err, "hiprtc (k_aukf): "), "aukf_prepare(dynamics_w of another signature)", err);
    printf("%d failed\n", failed);
    return failed;
}
