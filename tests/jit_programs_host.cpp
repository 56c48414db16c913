// jit_programs_host.cpp — every run-time compile path of libllpf_hip.so, driven without a device (tests/test_jit_programs.py).
// hiprtc cross-compiles for gfx950 when no device is visible; nothing is loaded or launched.  The entry points are the engine's own
// (csrc/engine.hpp, namespace llpf), declared here so that the program needs neither the HIP headers nor a device compiler.
// Build: c++ -std=c++17 -I <root>/include jit_programs_host.cpp -L <package> -lllpf_hip -Wl,-rpath,<package> -o jit_programs_host
// Prints one line per check; the exit status is the number of failed checks.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "llpf.h"

namespace llpf {
int ukf_prepare(int model_id, int nx, int ny, std::string& err);
int ukf_smooth_prepare(int model_id, int nx, int ny, std::string& err);
int ekf_prepare(int model_id, int nx, int ny, std::string& err);
int iekf_prepare(int model_id, int nx, int ny, std::string& err);
int simulate_prepare(int model_id, std::string& err);
int jit_builtin_lg(int nx, int ny, std::string& err);
int jit_prepare_rbfull(int fn_kind, int nn, int nl, int ny, std::string& err);
}  // namespace llpf

// a damped pendulum with neither dynamics_jac nor measurement_jac: the particle filter's kernels compile, k_ekf cannot
static const char* const PENDULUM_NO_JAC = R"SRC(
// tests/jit_programs_host.cpp
struct UserModel {
    static constexpr bool RB = false;
    double g_over_l, damp, dt;
    DEV void prepare(const ModelD* m, const double* u, double t) { g_over_l = m->qt[0]; damp = m->qt[1]; dt = m->Ts; }
    DEV void dynamics(const double* x, double* out) const {
        out[0] = x[0] + dt * x[1];
        out[1] = x[1] - dt * (g_over_l * x[0] + damp * x[1]);
    }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0]; }
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
    int lg51 = -1;
    // every path compiles, and the second call finds what the first one left
    for (int round = 0; round < 2; ++round) {
        const char* again = round ? " (again)" : "";
        err.clear(); check(ukf_prepare(LG, 5, 1, err) == 0, (std::string("ukf_prepare(LG, 5, 1)") + again).c_str(), err);
        err.clear(); check(ukf_smooth_prepare(LG, 5, 1, err) == 0, (std::string("ukf_smooth_prepare(LG, 5, 1)") + again).c_str(), err);
        err.clear(); check(ekf_prepare(LG, 5, 1, err) == 0, (std::string("ekf_prepare(LG, 5, 1)") + again).c_str(), err);
        err.clear(); check(iekf_prepare(LG, 5, 1, err) == 0, (std::string("iekf_prepare(LG, 5, 1)") + again).c_str(), err);
        err.clear();
        const int id = jit_builtin_lg(5, 1, err);
        check(id >= LLPF_MODEL_USER_BASE && (round == 0 || id == lg51), (std::string("jit_builtin_lg(5, 1)") + again).c_str(), err);
        lg51 = id;
        err.clear(); check(simulate_prepare(id, err) == 0, (std::string("simulate_prepare(LinGauss<5, 1>)") + again).c_str(), err);
        err.clear(); check(jit_prepare_rbfull(0, 2, 4, 2, err) == 0, (std::string("jit_prepare_rbfull(0, 2, 4, 2)") + again).c_str(), err);
    }
    // the precompiled shapes need no program: 0, and nothing said
    err.clear();
    check(ukf_prepare(LG, 4, 4, err) == 0 && ukf_smooth_prepare(LG, 1, 1, err) == 0 && ekf_prepare(LG, 2, 3, err) == 0 && iekf_prepare(LG, 3, 2, err) == 0 &&
              ukf_prepare(QT, 4, 2, err) == 0 && ukf_smooth_prepare(QT, 4, 2, err) == 0 && ekf_prepare(QT, 4, 2, err) == 0 && iekf_prepare(QT, 4, 2, err) == 0 &&
              simulate_prepare(LG, err) == 0 && simulate_prepare(QT, err) == 0 && err.empty(),
          "precompiled shapes", err);
    // an id nobody compiled
    const int nobody = LLPF_MODEL_USER_BASE + 900;
    const std::string at_dims = "unknown model id " + std::to_string(nobody) + " at these dimensions";
    err.clear(); check(ukf_prepare(nobody, 2, 1, err) == -1 && err == at_dims, "ukf_prepare(unknown id)", err);
    err.clear(); check(ukf_smooth_prepare(nobody, 2, 1, err) == -1 && err == at_dims, "ukf_smooth_prepare(unknown id)", err);
    err.clear(); check(ekf_prepare(nobody, 2, 1, err) == -1 && err == at_dims, "ekf_prepare(unknown id)", err);
    err.clear(); check(iekf_prepare(nobody, 2, 1, err) == -1 && err == at_dims, "iekf_prepare(unknown id)", err);
    err.clear(); check(simulate_prepare(nobody, err) == -1 && err == "unknown model id " + std::to_string(nobody), "simulate_prepare(unknown id)", err);
    // a model the extended filter cannot be compiled for: the log comes back under the kernel's name
    setenv("LLPF_JIT_COMPILE_ONLY", "1", 1);
    int32_t pend = -1;
    const int rc = llpf_model_compile(PENDULUM_NO_JAC, 2, 1, &pend);
    check(rc == LLPF_OK && pend >= LLPF_MODEL_USER_BASE, "llpf_model_compile(pendulum without Jacobians)", rc == LLPF_OK ? "" : llpf_last_error());
    err.clear(); check(ekf_prepare(pend, 2, 1, err) == -1 && starts_with(err, "hiprtc (k_ekf): "), "ekf_prepare(pendulum without Jacobians)", err);
    err.clear(); check(iekf_prepare(pend, 2, 1, err) == -1 && starts_with(err, "hiprtc (k_ekf, iterated): "), "iekf_prepare(pendulum without Jacobians)", err);
    err.clear(); check(ekf_prepare(pend, 3, 1, err) == -1 && err == "unknown model id " + std::to_string(pend) + " at these dimensions", "ekf_prepare(pendulum, other dimensions)", err);
    err.clear(); check(ukf_prepare(pend, 2, 1, err) == 0, "ukf_prepare(pendulum)", err);
    err.clear(); check(simulate_prepare(pend, err) == 0, "simulate_prepare(pendulum)", err);
    printf("%d failed\n", failed);
    return failed;
}
