// capi.hip — the C ABI declared in include/llpf.h: the error slot, the exception barrier and the table of exports.  An export checks its
// handle, defaults an output and makes one call; what it calls is host/*.hpp, included below into this one translation unit.
//
// There is deliberately NO CPU implementation behind these entry points: without a gfx950 device every
// constructor fails with LLPF_ERR_NO_DEVICE (host/bank.hpp: need_device).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "engine.hpp"
#include "shared/llpf_rbkf.h"
#include "shared/llpf_kalman.h"
#include "shared/llpf_sqkf.h"
#include "shared/llpf_imm.h"
#include "shared/llpf_ukf.h"
#include "shared/llpf_aukf.h"
#include "shared/llpf_ekf.h"
#include "shared/llpf_sqekf.h"
#include "shared/llpf_enkf.h"

using namespace llpf;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

// (noexcept: the message is dropped, never the status, if even the copy of the message cannot be allocated)
static int fail(int code, const std::string& msg) noexcept {
    try { g_err = msg; } catch (...) { g_err.clear(); }
    return code;
}
static int fail(int code, const char* msg) noexcept {
    try { g_err = msg; } catch (...) { g_err.clear(); }
    return code;
}

// The barrier include/llpf.h promises ("no C++ exception crosses the ABI"; SURVEY §8(b) Errors row; the reference turns a throw
// inside the likelihood into -Inf, src/smoothing.jl:275-279, never into a dead session).  Every export is a function-try-block
//     int llpf_name(...) LLPF_TRY { ... } LLPF_GUARD (llpf_name)
// whose handler maps what the host code can throw (std::vector / std::string / std::thread / the hiprtc cache) to a status.
// Building the message can itself run out of memory: then the status stands with a static message.
static int guard_catch(const char* fn) noexcept {
    int code = LLPF_ERR_INTERNAL;
    try {
        try { throw; }
        catch (const std::bad_alloc&) { code = LLPF_ERR_ALLOC; return fail(code, std::string(fn) + ": out of host memory"); }
        catch (const std::length_error& e) { code = LLPF_ERR_ALLOC; return fail(code, std::string(fn) + ": a size beyond what can be allocated (" + e.what() + ")"); }
        catch (const std::exception& e) { return fail(code, std::string(fn) + ": " + e.what()); }
        catch (...) { return fail(code, std::string(fn) + ": unknown exception"); }
    } catch (...) {
        return fail(code, code == LLPF_ERR_ALLOC ? "out of host memory" : "internal error");
    }
}
#define LLPF_TRY try
#define LLPF_GUARD(name) catch (...) { return guard_catch(#name); }

// Fault injection for the tests of that barrier: LLPF_TEST_THROW="<kind>:<site>", kind alloc | error | other; read at a handful of
// host-side sites (one getenv per API call, none per timestep).
static void test_throw(const char* site) {
    const char* e = getenv("LLPF_TEST_THROW");
    if (!e) return;
    const char* colon = strchr(e, ':');
    if (!colon || strcmp(colon + 1, site) != 0) return;
    if (!strncmp(e, "alloc", 5)) throw std::bad_alloc();
    if (!strncmp(e, "error", 5)) throw std::runtime_error(std::string("injected at ") + site);
    throw 42;
}
// (a failed runtime call also leaves its code in the runtime's "last error", which the next launch wrapper's hipGetLastError() would
//  report as its own — a refused hipMalloc used to poison the handle's next, unrelated call: cleared here; out of memory is LLPF_ERR_ALLOC)
#define HIPC(expr)                                                                                   \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            (void)hipGetLastError();                                                                 \
            return fail(_e == hipErrorOutOfMemory ? LLPF_ERR_ALLOC : LLPF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
        }                                                                                            \
    } while (0)
#define CHK(expr)                                                                                    \
    do {                                                                                             \
        int _c = (expr);                                                                             \
        if (_c != LLPF_OK) return _c;                                                                \
    } while (0)
#define NEEDF(f) if (!(f)) return fail(LLPF_ERR_ARG, "null handle")

#include "host/densities.hpp"
#include "host/run_plan.hpp"
#include "host/bank.hpp"
#include "host/fallback.hpp"
#include "host/rbkf.hpp"
#include "host/steps.hpp"
#include "host/run.hpp"
#include "host/aux.hpp"
#include "host/smooth.hpp"
#include "host/access.hpp"
#include "host/primitives.hpp"
#include "host/mbank.hpp"
#include "host/pipe.hpp"
#include "host/simulate.hpp"
#include "host/kfbank.hpp"
#include "host/kalman.hpp"
#include "host/sqkf.hpp"
#include "host/imm.hpp"
#include "host/ukf.hpp"
#include "host/aukf.hpp"
#include "host/ekf.hpp"
#include "host/sqekf.hpp"
#include "host/enkf.hpp"

// A new handle: `build` fills it, a status other than LLPF_OK frees it again.  No handler here: what build throws is caught by the
// export's own function-try-block (which names the export), the half-built handle freed on the way.
template <class H, class Build>
static int make_handle(H** out, Build build) {
    if (!out) return fail(LLPF_ERR_ARG, "null out pointer");
    *out = nullptr;
    std::unique_ptr<H> h(new (std::nothrow) H());
    if (!h) return fail(LLPF_ERR_ALLOC, "out of host memory");
    CHK(build(*h));
    *out = h.release();
    return LLPF_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* llpf_last_error(void) { return g_err.c_str(); }      // (noexcept by construction: the only export without a status)

int llpf_version(int32_t* major, int32_t* minor) LLPF_TRY {
    if (major) *major = LLPF_VERSION_MAJOR;
    if (minor) *minor = LLPF_VERSION_MINOR;
    return LLPF_OK;
} LLPF_GUARD(llpf_version)

int llpf_device_count(int32_t* n) LLPF_TRY { if (n) *n = device_count(); return LLPF_OK; } LLPF_GUARD(llpf_device_count)

int llpf_create(const llpf_config* cfg, llpf_filter** out) LLPF_TRY {
    return make_handle(out, [&](llpf_filter& f) { return bank_create(cfg, nullptr, 1, f.bank); });
} LLPF_GUARD(llpf_create)
int llpf_destroy(llpf_filter* f) LLPF_TRY { delete f; return LLPF_OK; } LLPF_GUARD(llpf_destroy)

int llpf_reset(llpf_filter* f) LLPF_TRY { NEEDF(f); return bank_reset(f->bank); } LLPF_GUARD(llpf_reset)
int llpf_seed(llpf_filter* f, uint64_t seed) LLPF_TRY { NEEDF(f); return bank_seed(f->bank, seed); } LLPF_GUARD(llpf_seed)
int llpf_set_model(llpf_filter* f, const llpf_model* model) LLPF_TRY { NEEDF(f); return bank_set_models(f->bank, model); } LLPF_GUARD(llpf_set_model)

int llpf_correct(llpf_filter* f, const double* u, const double* y, double t, double* ll) LLPF_TRY {
    NEEDF(f);
    double l = 0.0;
    int rc = bank_correct(f->bank, u, y, t, &l);
    if (ll) *ll = l;
    return rc;
} LLPF_GUARD(llpf_correct)
int llpf_predict(llpf_filter* f, const double* u, double t) LLPF_TRY { NEEDF(f); return bank_predict(f->bank, u, t); } LLPF_GUARD(llpf_predict)
int llpf_update(llpf_filter* f, const double* u, const double* y, double t, double* ll) LLPF_TRY {
    NEEDF(f);
    int rc = llpf_correct(f, u, y, t, ll);
    if (rc != LLPF_OK) return rc;
    return bank_predict(f->bank, u, t);
} LLPF_GUARD(llpf_update)

int llpf_run(llpf_filter* f, const double* U, const double* Y, int64_t T, double t_index0,
             double* ll_total, const llpf_run_outputs* o) LLPF_TRY {
    NEEDF(f);
    double lt = 0.0;
    int rc = bank_run(f->bank, U, Y, T, t_index0, &lt, o ? *o : llpf_run_outputs{});
    if (ll_total) *ll_total = lt;
    return rc;
} LLPF_GUARD(llpf_run)

int llpf_aux_correct(llpf_filter* f, double* ll) LLPF_TRY {
    NEEDF(f);
    double l = 0.0;
    int rc = bank_aux_correct(f->bank, &l, AuxOuts{}, 0);
    if (ll) *ll = l;
    return rc;
} LLPF_GUARD(llpf_aux_correct)
int llpf_aux_predict(llpf_filter* f, const double* u, const double* y1, double t) LLPF_TRY { NEEDF(f); return bank_aux_predict(f->bank, u, y1, t); } LLPF_GUARD(llpf_aux_predict)
int llpf_aux_update(llpf_filter* f, const double* u, const double* y1, double t, double* ll) LLPF_TRY {
    NEEDF(f);
    int rc = llpf_aux_correct(f, ll);
    if (rc != LLPF_OK) return rc;
    return bank_aux_predict(f->bank, u, y1, t);
} LLPF_GUARD(llpf_aux_update)
int llpf_aux_run(llpf_filter* f, const double* U, const double* Y, int64_t T, int32_t mode,
                 double* ll_total, const llpf_run_outputs* o) LLPF_TRY {
    NEEDF(f);
    if (o && (o->xcov || o->xquant)) return fail(LLPF_ERR_ARG, "the xcov / xquant outputs are provided by llpf_run only");
    double lt = 0.0;
    int rc = bank_aux_run(f->bank, U, Y, T, mode, &lt, o ? *o : llpf_run_outputs{});
    if (ll_total) *ll_total = lt;
    return rc;
} LLPF_GUARD(llpf_aux_run)
int llpf_bank_aux_run(llpf_bank* b, const double* U, const double* Y, int64_t T, int32_t mode,
                      double* ll_total, double* ll_steps) LLPF_TRY {
    NEEDF(b);
    llpf_run_outputs o{};
    o.ll_steps = ll_steps;
    return bank_aux_run(b->bank, U, Y, T, mode, ll_total, o);
} LLPF_GUARD(llpf_bank_aux_run)

int llpf_simulate(llpf_filter* f, int64_t M, int64_t T, const double* U, int32_t u_per_trajectory, double t_index0,
                  uint64_t seed, uint32_t step0, int32_t flags, double* X, double* Y) LLPF_TRY {
    NEEDF(f);
    return bank_simulate(f->bank, M, T, U, u_per_trajectory, t_index0, seed, step0, flags, X, Y);
} LLPF_GUARD(llpf_simulate)
int llpf_bank_simulate(llpf_bank* b, int64_t M, int64_t T, const double* U, int32_t u_per_trajectory, double t_index0,
                       uint64_t seed, uint32_t step0, int32_t flags, double* X, double* Y) LLPF_TRY {
    NEEDF(b);
    return bank_simulate(b->bank, M, T, U, u_per_trajectory, t_index0, seed, step0, flags, X, Y);
} LLPF_GUARD(llpf_bank_simulate)

// ---- banks of Kalman filters (host/kfbank.hpp, host/kalman.hpp) ----
int llpf_kalman_bank_create(int32_t device, const llpf_model* models, const double* D, int32_t n_filters, llpf_kalman_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_kalman_bank& b) { return kalman_create(device, models, D, n_filters, b); });
} LLPF_GUARD(llpf_kalman_bank_create)
int llpf_kalman_bank_destroy(llpf_kalman_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_kalman_bank_destroy)
int llpf_kalman_bank_reset(llpf_kalman_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_kalman_bank_reset)
int llpf_kalman_bank_set_models(llpf_kalman_bank* b, const llpf_model* models, const double* D) LLPF_TRY {
    NEEDF(b);
    return kalman_set_models(*b, models, D);
} LLPF_GUARD(llpf_kalman_bank_set_models)
int llpf_kalman_bank_run(llpf_kalman_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                         const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return kalman_run(*b, U, Y, T, per_filter, ll_total, out);
} LLPF_GUARD(llpf_kalman_bank_run)
int llpf_kalman_bank_smooth(llpf_kalman_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                            const llpf_kalman_outputs* forward, const llpf_kalman_smooth_outputs* out) LLPF_TRY {
    NEEDF(b);
    return kalman_smooth(*b, U, Y, T, per_filter, ll_total, forward, out);
} LLPF_GUARD(llpf_kalman_bank_smooth)
int llpf_kalman_bank_get_state(llpf_kalman_bank* b, double* x, double* R) LLPF_TRY { NEEDF(b); return kf_get_state(*b, x, R); } LLPF_GUARD(llpf_kalman_bank_get_state)
int llpf_kalman_bank_set_state(llpf_kalman_bank* b, const double* x, const double* R) LLPF_TRY { NEEDF(b); return kf_set_state(*b, x, R); } LLPF_GUARD(llpf_kalman_bank_set_state)

// ---- banks of square-root Kalman filters (host/kfbank.hpp, host/sqkf.hpp) ----
int llpf_sqkf_bank_create(int32_t device, const llpf_model* models, const double* D, int32_t n_filters, llpf_sqkf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_sqkf_bank& b) { return sqkf_create(device, models, D, n_filters, b); });
} LLPF_GUARD(llpf_sqkf_bank_create)
int llpf_sqkf_bank_destroy(llpf_sqkf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_sqkf_bank_destroy)
int llpf_sqkf_bank_reset(llpf_sqkf_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_sqkf_bank_reset)
int llpf_sqkf_bank_set_models(llpf_sqkf_bank* b, const llpf_model* models, const double* D) LLPF_TRY {
    NEEDF(b);
    return sqkf_set_models(*b, models, D);
} LLPF_GUARD(llpf_sqkf_bank_set_models)
int llpf_sqkf_bank_run(llpf_sqkf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                       const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return sqkf_run(*b, U, Y, T, per_filter, ll_total, out);
} LLPF_GUARD(llpf_sqkf_bank_run)
int llpf_sqkf_bank_get_state(llpf_sqkf_bank* b, double* x, double* R, double* L) LLPF_TRY { NEEDF(b); return sqkf_get_state(*b, x, R, L); } LLPF_GUARD(llpf_sqkf_bank_get_state)
int llpf_sqkf_bank_set_state(llpf_sqkf_bank* b, const double* x, const double* R, const double* L) LLPF_TRY { NEEDF(b); return sqkf_set_state(*b, x, R, L); } LLPF_GUARD(llpf_sqkf_bank_set_state)

// ---- banks of IMM filters over Kalman, extended Kalman or unscented Kalman filters (host/kfbank.hpp, host/imm.hpp) ----
int llpf_imm_bank_create(int32_t device, const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t n_filters,
                         int32_t n_modes, int32_t flags, llpf_imm_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_imm_bank& b) { return imm_create(device, models, D, P, mu0, n_filters, n_modes, flags, b); });
} LLPF_GUARD(llpf_imm_bank_create)
int llpf_imm_bank_create_unscented(int32_t device, const llpf_model* models, const double* P, const double* mu0, int32_t n_filters,
                                   int32_t n_modes, int32_t flags, const llpf_ukf_weights* w, llpf_imm_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_imm_bank& b) { return imm_create_unscented(device, models, P, mu0, n_filters, n_modes, flags, w, b); });
} LLPF_GUARD(llpf_imm_bank_create_unscented)
int llpf_imm_bank_set_weights(llpf_imm_bank* b, const llpf_ukf_weights* w) LLPF_TRY { NEEDF(b); return imm_set_weights(*b, w); } LLPF_GUARD(llpf_imm_bank_set_weights)
int llpf_imm_bank_destroy(llpf_imm_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_imm_bank_destroy)
int llpf_imm_bank_reset(llpf_imm_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_imm_bank_reset)
int llpf_imm_bank_set_models(llpf_imm_bank* b, const llpf_model* models, const double* D, const double* P, const double* mu0) LLPF_TRY {
    NEEDF(b);
    return imm_set_models(*b, models, D, P, mu0);
} LLPF_GUARD(llpf_imm_bank_set_models)
int llpf_imm_bank_run(llpf_imm_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                      const llpf_imm_outputs* out) LLPF_TRY {
    NEEDF(b);
    return imm_run(*b, U, Y, T, per_filter, 0.0, ll_total, out);
} LLPF_GUARD(llpf_imm_bank_run)
int llpf_imm_bank_run_at(llpf_imm_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                         const llpf_imm_outputs* out) LLPF_TRY {
    CHK(imm_check_time(t_index0));
    NEEDF(b);
    return imm_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_imm_bank_run_at)
int llpf_imm_bank_get_state(llpf_imm_bank* b, double* x, double* R, double* mu, double* x_modes, double* R_modes) LLPF_TRY {
    NEEDF(b);
    return imm_get_state(*b, x, R, mu, x_modes, R_modes);
} LLPF_GUARD(llpf_imm_bank_get_state)
int llpf_imm_bank_set_state(llpf_imm_bank* b, const double* mu, const double* x_modes, const double* R_modes) LLPF_TRY {
    NEEDF(b);
    return imm_set_state(*b, mu, x_modes, R_modes);
} LLPF_GUARD(llpf_imm_bank_set_state)

// ---- banks of unscented Kalman filters (host/kfbank.hpp, host/ukf.hpp) ----
int llpf_ukf_bank_create(int32_t device, const llpf_model* models, int32_t n_filters, const llpf_ukf_weights* w, llpf_ukf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_ukf_bank& b) { return ukf_create(device, models, n_filters, w, b); });
} LLPF_GUARD(llpf_ukf_bank_create)
int llpf_ukf_bank_destroy(llpf_ukf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_ukf_bank_destroy)
int llpf_ukf_bank_reset(llpf_ukf_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_ukf_bank_reset)
int llpf_ukf_bank_set_models(llpf_ukf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return kf_model_set_models(*b, models); } LLPF_GUARD(llpf_ukf_bank_set_models)
int llpf_ukf_bank_set_weights(llpf_ukf_bank* b, const llpf_ukf_weights* w) LLPF_TRY { NEEDF(b); return ukf_set_weights(*b, w); } LLPF_GUARD(llpf_ukf_bank_set_weights)
int llpf_ukf_bank_run(llpf_ukf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                      const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return ukf_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_ukf_bank_run)
int llpf_ukf_bank_smooth(llpf_ukf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                         const llpf_kalman_outputs* forward, const llpf_kalman_smooth_outputs* out) LLPF_TRY {
    NEEDF(b);
    return ukf_smooth(*b, U, Y, T, per_filter, t_index0, ll_total, forward, out);
} LLPF_GUARD(llpf_ukf_bank_smooth)
int llpf_ukf_bank_get_state(llpf_ukf_bank* b, double* x, double* R) LLPF_TRY { NEEDF(b); return kf_get_state(*b, x, R); } LLPF_GUARD(llpf_ukf_bank_get_state)
int llpf_ukf_bank_set_state(llpf_ukf_bank* b, const double* x, const double* R) LLPF_TRY { NEEDF(b); return kf_set_state(*b, x, R); } LLPF_GUARD(llpf_ukf_bank_set_state)

// ---- banks of extended Kalman filters (host/kfbank.hpp, host/ekf.hpp) ----
int llpf_ekf_bank_create(int32_t device, const llpf_model* models, int32_t n_filters, llpf_ekf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_ekf_bank& b) { return kf_model_create(b, device, models, n_filters, "ekf_create", ekf_prepare); });
} LLPF_GUARD(llpf_ekf_bank_create)
int llpf_ekf_bank_destroy(llpf_ekf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_ekf_bank_destroy)
int llpf_ekf_bank_reset(llpf_ekf_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_ekf_bank_reset)
int llpf_ekf_bank_set_models(llpf_ekf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return kf_model_set_models(*b, models); } LLPF_GUARD(llpf_ekf_bank_set_models)
int llpf_ekf_bank_set_iterations(llpf_ekf_bank* b, int32_t maxiters, double epsilon) LLPF_TRY {
    CHK(ekf_check_iterations(maxiters, epsilon));      // (the two numbers before the handle: their messages do not wait for a bank)
    if (!b) return fail(LLPF_ERR_ARG, "ekf: null handle");
    return ekf_set_iterations(*b, maxiters, epsilon);
} LLPF_GUARD(llpf_ekf_bank_set_iterations)
int llpf_ekf_bank_run(llpf_ekf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                      const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return ekf_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_ekf_bank_run)
int llpf_ekf_bank_get_state(llpf_ekf_bank* b, double* x, double* R) LLPF_TRY { NEEDF(b); return kf_get_state(*b, x, R); } LLPF_GUARD(llpf_ekf_bank_get_state)
int llpf_ekf_bank_set_state(llpf_ekf_bank* b, const double* x, const double* R) LLPF_TRY { NEEDF(b); return kf_set_state(*b, x, R); } LLPF_GUARD(llpf_ekf_bank_set_state)

// ---- banks of unscented Kalman filters with augmented process noise (host/kfbank.hpp, host/aukf.hpp) ----
int llpf_aukf_bank_create(int32_t device, const llpf_model* models, int32_t n_filters, const llpf_ukf_weights* w_measurement,
                          const llpf_ukf_weights* w_dynamics, llpf_aukf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_aukf_bank& b) { return aukf_create(device, models, n_filters, w_measurement, w_dynamics, b); });
} LLPF_GUARD(llpf_aukf_bank_create)
int llpf_aukf_bank_destroy(llpf_aukf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_aukf_bank_destroy)
int llpf_aukf_bank_reset(llpf_aukf_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_aukf_bank_reset)
int llpf_aukf_bank_set_models(llpf_aukf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return kf_model_set_models(*b, models); } LLPF_GUARD(llpf_aukf_bank_set_models)
int llpf_aukf_bank_set_weights(llpf_aukf_bank* b, const llpf_ukf_weights* w_measurement, const llpf_ukf_weights* w_dynamics) LLPF_TRY {
    NEEDF(b);
    return aukf_set_weights(*b, w_measurement, w_dynamics);
} LLPF_GUARD(llpf_aukf_bank_set_weights)
int llpf_aukf_bank_run(llpf_aukf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                       const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return aukf_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_aukf_bank_run)
int llpf_aukf_bank_get_state(llpf_aukf_bank* b, double* x, double* R) LLPF_TRY { NEEDF(b); return kf_get_state(*b, x, R); } LLPF_GUARD(llpf_aukf_bank_get_state)
int llpf_aukf_bank_set_state(llpf_aukf_bank* b, const double* x, const double* R) LLPF_TRY { NEEDF(b); return kf_set_state(*b, x, R); } LLPF_GUARD(llpf_aukf_bank_set_state)

// ---- banks of square-root extended Kalman filters (host/kfbank.hpp, host/sqekf.hpp) ----
int llpf_sqekf_bank_create(int32_t device, const llpf_model* models, int32_t n_filters, llpf_sqekf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_sqekf_bank& b) { return sqekf_create(b, device, models, n_filters); });
} LLPF_GUARD(llpf_sqekf_bank_create)
int llpf_sqekf_bank_destroy(llpf_sqekf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_sqekf_bank_destroy)
int llpf_sqekf_bank_reset(llpf_sqekf_bank* b) LLPF_TRY { NEEDF(b); return kf_reset(*b); } LLPF_GUARD(llpf_sqekf_bank_reset)
int llpf_sqekf_bank_set_models(llpf_sqekf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return sqekf_set_models(*b, models); } LLPF_GUARD(llpf_sqekf_bank_set_models)
int llpf_sqekf_bank_run(llpf_sqekf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                        const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return sqekf_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_sqekf_bank_run)
int llpf_sqekf_bank_get_state(llpf_sqekf_bank* b, double* x, double* R, double* L) LLPF_TRY { NEEDF(b); return sqkf_get_state(*b, x, R, L); } LLPF_GUARD(llpf_sqekf_bank_get_state)
int llpf_sqekf_bank_set_state(llpf_sqekf_bank* b, const double* x, const double* R, const double* L) LLPF_TRY { NEEDF(b); return sqkf_set_state(*b, x, R, L); } LLPF_GUARD(llpf_sqekf_bank_set_state)

// ---- banks of ensemble Kalman filters (host/kfbank.hpp, host/enkf.hpp) ----
int llpf_enkf_bank_create(int32_t device, const llpf_model* models, int32_t n_filters, int32_t n_members, uint64_t seed, llpf_enkf_bank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_enkf_bank& b) { return enkf_create(b, device, models, n_filters, n_members, seed); });
} LLPF_GUARD(llpf_enkf_bank_create)
int llpf_enkf_bank_destroy(llpf_enkf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_enkf_bank_destroy)
int llpf_enkf_bank_reset(llpf_enkf_bank* b) LLPF_TRY { NEEDF(b); return enkf_reset(*b); } LLPF_GUARD(llpf_enkf_bank_reset)
int llpf_enkf_bank_seed(llpf_enkf_bank* b, uint64_t seed) LLPF_TRY { NEEDF(b); return enkf_seed(*b, seed); } LLPF_GUARD(llpf_enkf_bank_seed)
int llpf_enkf_bank_set_models(llpf_enkf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return kf_model_set_models(*b, models); } LLPF_GUARD(llpf_enkf_bank_set_models)
int llpf_enkf_bank_set_inflation(llpf_enkf_bank* b, double rho) LLPF_TRY {
    NEEDF(b);
    CHK(enkf_check_inflation(rho));
    b->rho = rho;
    return LLPF_OK;
} LLPF_GUARD(llpf_enkf_bank_set_inflation)
int llpf_enkf_bank_run(llpf_enkf_bank* b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                       const llpf_kalman_outputs* out) LLPF_TRY {
    NEEDF(b);
    return enkf_run(*b, U, Y, T, per_filter, t_index0, ll_total, out);
} LLPF_GUARD(llpf_enkf_bank_run)
int llpf_enkf_bank_correct(llpf_enkf_bank* b, const double* u, const double* y, int32_t per_filter, double t_index, double* ll, double* e) LLPF_TRY {
    NEEDF(b);
    return enkf_correct(*b, u, y, per_filter, t_index, ll, e);
} LLPF_GUARD(llpf_enkf_bank_correct)
int llpf_enkf_bank_predict(llpf_enkf_bank* b, const double* u, int32_t per_filter, double t_index) LLPF_TRY {
    NEEDF(b);
    return enkf_predict(*b, u, per_filter, t_index);
} LLPF_GUARD(llpf_enkf_bank_predict)
int llpf_enkf_bank_get_state(llpf_enkf_bank* b, double* x, double* R) LLPF_TRY { NEEDF(b); return kf_get_state(*b, x, R); } LLPF_GUARD(llpf_enkf_bank_get_state)
int llpf_enkf_bank_get_members(llpf_enkf_bank* b, double* X) LLPF_TRY { NEEDF(b); return enkf_get_members(*b, X); } LLPF_GUARD(llpf_enkf_bank_get_members)
int llpf_enkf_bank_set_members(llpf_enkf_bank* b, const double* X) LLPF_TRY { NEEDF(b); return enkf_set_members(*b, X); } LLPF_GUARD(llpf_enkf_bank_set_members)

// ---- the state of a filter (host/access.hpp) ----
int llpf_rb_get_covariance(llpf_filter* f, double* R) LLPF_TRY { NEEDF(f); return bank_rb_covariance(f->bank, R); } LLPF_GUARD(llpf_rb_get_covariance)
int llpf_rb_get_linear_state(llpf_filter* f, double* xl, double* R) LLPF_TRY { NEEDF(f); return bank_rb_linear_state(f->bank, xl, R); } LLPF_GUARD(llpf_rb_get_linear_state)

int llpf_smooth(llpf_filter* f, int64_t M, const double* U, int64_t T, const double* xf, const double* wf,
                const double* wef, double* xb, int64_t* idx) LLPF_TRY {
    NEEDF(f);
    return bank_smooth(f->bank, M, U, T, xf, wf, wef, xb, idx);
} LLPF_GUARD(llpf_smooth)

int llpf_num_particles(const llpf_filter* f, int64_t* n) LLPF_TRY { NEEDF(f); if (n) *n = f->bank.N; return LLPF_OK; } LLPF_GUARD(llpf_num_particles)
int llpf_index(const llpf_filter* f, int64_t* t) LLPF_TRY { NEEDF(f); if (t) *t = f->bank.t_index; return LLPF_OK; } LLPF_GUARD(llpf_index)
int llpf_set_index(llpf_filter* f, int64_t t) LLPF_TRY { NEEDF(f); f->bank.t_index = t; return LLPF_OK; } LLPF_GUARD(llpf_set_index)
int llpf_get_particles(llpf_filter* f, double* dst) LLPF_TRY { NEEDF(f); return bank_get_particles(f->bank, dst); } LLPF_GUARD(llpf_get_particles)
int llpf_get_weights(llpf_filter* f, double* dst) LLPF_TRY { NEEDF(f); return bank_get_w(f->bank, dst, false); } LLPF_GUARD(llpf_get_weights)
int llpf_get_expweights(llpf_filter* f, double* dst) LLPF_TRY { NEEDF(f); return bank_get_w(f->bank, dst, true); } LLPF_GUARD(llpf_get_expweights)
int llpf_get_ancestors(llpf_filter* f, int64_t* dst) LLPF_TRY { NEEDF(f); return bank_get_ancestors(f->bank, dst); } LLPF_GUARD(llpf_get_ancestors)
int llpf_get_bins(llpf_filter* f, double* dst) LLPF_TRY { NEEDF(f); return bank_get_bins(f->bank, dst); } LLPF_GUARD(llpf_get_bins)
int llpf_set_particles(llpf_filter* f, const double* src) LLPF_TRY { NEEDF(f); return bank_set_particles(f->bank, src); } LLPF_GUARD(llpf_set_particles)
int llpf_set_weights(llpf_filter* f, const double* w) LLPF_TRY { NEEDF(f); return bank_set_weights(f->bank, w); } LLPF_GUARD(llpf_set_weights)

int llpf_effective_particles(llpf_filter* f, double* ess) LLPF_TRY {
    NEEDF(f);
    FilterScal s;
    CHK(bank_scal0(f->bank, &s, true));
    if (ess) *ess = s.ess;
    return LLPF_OK;
} LLPF_GUARD(llpf_effective_particles)
int llpf_shouldresample(llpf_filter* f, int32_t* yes) LLPF_TRY {
    NEEDF(f);
    FilterScal s;
    CHK(bank_scal0(f->bank, &s, true));
    if (yes) *yes = s.do_resample;
    return LLPF_OK;
} LLPF_GUARD(llpf_shouldresample)
int llpf_last_resampled(llpf_filter* f, int32_t* yes) LLPF_TRY {
    NEEDF(f);
    FilterScal s;
    CHK(bank_scal0(f->bank, &s, false));
    if (yes) *yes = s.last_resampled;
    return LLPF_OK;
} LLPF_GUARD(llpf_last_resampled)
int llpf_maxw(llpf_filter* f, double* maxw) LLPF_TRY {
    NEEDF(f);
    FilterScal s;
    CHK(bank_scal0(f->bank, &s, false));
    if (maxw) *maxw = s.mtrue;
    return LLPF_OK;
} LLPF_GUARD(llpf_maxw)
int llpf_weighted_mean(llpf_filter* f, double* xh) LLPF_TRY { NEEDF(f); return bank_weighted_mean(f->bank, xh); } LLPF_GUARD(llpf_weighted_mean)
int llpf_weighted_cov(llpf_filter* f, double* cov) LLPF_TRY { NEEDF(f); return bank_weighted_cov(f->bank, cov); } LLPF_GUARD(llpf_weighted_cov)
int llpf_weighted_quantile(llpf_filter* f, const double* q, int32_t nq, double* out) LLPF_TRY {
    NEEDF(f);
    return bank_weighted_quantile(f->bank, q, nq, out);
} LLPF_GUARD(llpf_weighted_quantile)
int llpf_resample_count(llpf_filter* f, int64_t* n) LLPF_TRY { NEEDF(f); if (n) *n = f->bank.run_resamples; return LLPF_OK; } LLPF_GUARD(llpf_resample_count)
int llpf_last_run_stats(llpf_filter* f, int64_t* fused_launches, int64_t* source_side_timesteps, double* survivor_fraction) LLPF_TRY {
    NEEDF(f);
    if (fused_launches) *fused_launches = f->bank.last_run_launches;
    if (source_side_timesteps) *source_side_timesteps = f->bank.last_run_fx_steps;
    if (survivor_fraction) *survivor_fraction = f->bank.last_run_surv;
    return LLPF_OK;
} LLPF_GUARD(llpf_last_run_stats)
int llpf_last_run_form(llpf_filter* f, int32_t* weights_not_stored, int64_t* exact_redos) LLPF_TRY {
    NEEDF(f);
    if (weights_not_stored) *weights_not_stored = ((1 << f->bank.last_run_level) - 1) | (f->bank.last_run_skip_max ? 8 : 0);
    if (exact_redos) *exact_redos = f->bank.last_run_redos;
    return LLPF_OK;
} LLPF_GUARD(llpf_last_run_form)
int llpf_last_run_ms(llpf_filter* f, double* ms) LLPF_TRY { NEEDF(f); if (ms) *ms = f->bank.last_run_ms; return LLPF_OK; } LLPF_GUARD(llpf_last_run_ms)
int llpf_set_profiling(llpf_filter* f, int32_t on) LLPF_TRY { NEEDF(f); return set_prof(f->bank, on); } LLPF_GUARD(llpf_set_profiling)
int llpf_get_profile(llpf_filter* f, double* ms, int64_t* n) LLPF_TRY { NEEDF(f); return get_prof(f->bank, ms, n); } LLPF_GUARD(llpf_get_profile)

// ---- user-supplied models (kernels/jit.hpp) -----------------------------------------------------------
int llpf_model_traits(int32_t model_id, int32_t* traits) LLPF_TRY {
    if (!traits) return fail(LLPF_ERR_ARG, "null pointer");
    const int t = jit_model_traits(model_id);
    if (t < 0) return fail(LLPF_ERR_ARG, "llpf_model_traits: not the id of a run-time compiled model");
    *traits = t;
    return LLPF_OK;
} LLPF_GUARD(llpf_model_traits)
int llpf_model_compile(const char* device_src, int32_t nx, int32_t ny, int32_t* model_id) LLPF_TRY {
    if (!model_id) return fail(LLPF_ERR_ARG, "null output");
    *model_id = -1;
    // (LLPF_JIT_COMPILE_ONLY=1: the build check on a box without a GPU — hiprtc cross-compiles for gfx950; nothing can run)
    const char* co = getenv("LLPF_JIT_COMPILE_ONLY");
    if (!(co && atoi(co))) CHK(need_device());
    std::string err;
    const int id = jit_compile_user_model(device_src, nx, ny, err);
    if (id < 0) return fail(LLPF_ERR_ARG, err);
    *model_id = id;
    return LLPF_OK;
} LLPF_GUARD(llpf_model_compile)

// ---- banks ---------------------------------------------------------------------------------------
int llpf_bank_create(const llpf_config* base, const llpf_model* models, int32_t n_filters, llpf_bank** out) LLPF_TRY {
    // models == NULL: every filter uses base->model (Monte-Carlo replicas; seeds differ: seed + k)
    return make_handle(out, [&](llpf_bank& b) { return bank_create(base, models, n_filters, b.bank); });
} LLPF_GUARD(llpf_bank_create)
int llpf_bank_destroy(llpf_bank* b) LLPF_TRY { delete b; return LLPF_OK; } LLPF_GUARD(llpf_bank_destroy)
int llpf_bank_reset(llpf_bank* b) LLPF_TRY { NEEDF(b); return bank_reset(b->bank); } LLPF_GUARD(llpf_bank_reset)
int llpf_bank_seed(llpf_bank* b, uint64_t seed) LLPF_TRY { NEEDF(b); return bank_seed(b->bank, seed); } LLPF_GUARD(llpf_bank_seed)
int llpf_bank_set_models(llpf_bank* b, const llpf_model* models) LLPF_TRY { NEEDF(b); return bank_set_models(b->bank, models); } LLPF_GUARD(llpf_bank_set_models)
int llpf_bank_run(llpf_bank* b, const double* U, const double* Y, int64_t T, double t_index0,
                  double* ll_total, double* ll_steps) LLPF_TRY {
    NEEDF(b);
    llpf_run_outputs o{};
    o.ll_steps = ll_steps;
    return bank_run(b->bank, U, Y, T, t_index0, ll_total, o);
} LLPF_GUARD(llpf_bank_run)
int llpf_bank_run_multi(llpf_bank* b, const double* U, const double* Y, int64_t T, double t_index0,
                        double* ll_total, double* ll_steps, double* xmean) LLPF_TRY {
    NEEDF(b);
    llpf_run_outputs o{};
    o.ll_steps = ll_steps; o.xmean = xmean;
    return bank_run(b->bank, U, Y, T, t_index0, ll_total, o, true);
} LLPF_GUARD(llpf_bank_run_multi)
int llpf_bank_set_profiling(llpf_bank* b, int32_t on) LLPF_TRY { NEEDF(b); return set_prof(b->bank, on); } LLPF_GUARD(llpf_bank_set_profiling)
int llpf_bank_get_profile(llpf_bank* b, double* ms, int64_t* n) LLPF_TRY { NEEDF(b); return get_prof(b->bank, ms, n); } LLPF_GUARD(llpf_bank_get_profile)
int llpf_bank_resample_count(llpf_bank* b, int64_t* n) LLPF_TRY { NEEDF(b); if (n) *n = b->bank.run_resamples; return LLPF_OK; } LLPF_GUARD(llpf_bank_resample_count)
int llpf_bank_last_run_ms(llpf_bank* b, double* ms) LLPF_TRY { NEEDF(b); if (ms) *ms = b->bank.last_run_ms; return LLPF_OK; } LLPF_GUARD(llpf_bank_last_run_ms)

// ---- sweeps sharded over the GPUs of a node (host/mbank.hpp) ---------------------------------------
int llpf_mbank_create(const llpf_config* base, const llpf_model* models, int32_t n_filters, const int32_t* devices,
                      int32_t n_devices, llpf_mbank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_mbank& m) { return mbank_create(m, base, models, n_filters, devices, n_devices); });
} LLPF_GUARD(llpf_mbank_create)
int llpf_mbank_unique_id(uint8_t* id) LLPF_TRY { return mbank_unique_id(id); } LLPF_GUARD(llpf_mbank_unique_id)
int llpf_mbank_partition(int32_t n_filters, int32_t shard, int32_t n_shards, int32_t* owned, int32_t* n_owned) LLPF_TRY {
    return mbank_partition(n_filters, shard, n_shards, owned, n_owned);
} LLPF_GUARD(llpf_mbank_partition)
int llpf_mbank_create_rank(const llpf_config* base, const llpf_model* models, int32_t n_filters, int32_t rank, int32_t world,
                           const uint8_t* id, llpf_mbank** out) LLPF_TRY {
    return make_handle(out, [&](llpf_mbank& m) { return mbank_create_rank(m, base, models, n_filters, rank, world, id); });
} LLPF_GUARD(llpf_mbank_create_rank)
int llpf_mbank_destroy(llpf_mbank* m) LLPF_TRY { delete m; return LLPF_OK; } LLPF_GUARD(llpf_mbank_destroy)
int llpf_mbank_reset(llpf_mbank* m) LLPF_TRY { NEEDF(m); return mbank_reset(*m); } LLPF_GUARD(llpf_mbank_reset)
int llpf_mbank_seed(llpf_mbank* m, uint64_t seed) LLPF_TRY { NEEDF(m); return mbank_seed(*m, seed); } LLPF_GUARD(llpf_mbank_seed)
int llpf_mbank_set_models(llpf_mbank* m, const llpf_model* models) LLPF_TRY { NEEDF(m); return mbank_set_models(*m, models); } LLPF_GUARD(llpf_mbank_set_models)
int llpf_mbank_run(llpf_mbank* m, const double* U, const double* Y, int64_t T, double t_index0, double* ll_total, double* ll_sum) LLPF_TRY {
    NEEDF(m);
    return mbank_run(*m, U, Y, T, t_index0, ll_total, ll_sum, false, 0);
} LLPF_GUARD(llpf_mbank_run)
int llpf_mbank_aux_run(llpf_mbank* m, const double* U, const double* Y, int64_t T, int32_t mode, double* ll_total, double* ll_sum) LLPF_TRY {
    NEEDF(m);
    return mbank_run(*m, U, Y, T, 0.0, ll_total, ll_sum, true, mode);
} LLPF_GUARD(llpf_mbank_aux_run)
int llpf_mbank_info(llpf_mbank* m, llpf_mbank_info_t* info) LLPF_TRY { NEEDF(m); return mbank_info(*m, info); } LLPF_GUARD(llpf_mbank_info)
int llpf_mbank_local_devices(llpf_mbank* m, int32_t* devices) LLPF_TRY { NEEDF(m); return mbank_local_devices(*m, devices); } LLPF_GUARD(llpf_mbank_local_devices)
int llpf_mbank_set_profiling(llpf_mbank* m, int32_t on) LLPF_TRY { NEEDF(m); return mbank_set_prof(*m, on); } LLPF_GUARD(llpf_mbank_set_profiling)
int llpf_mbank_get_profile(llpf_mbank* m, int32_t local_shard, double* ms, int64_t* n) LLPF_TRY {
    NEEDF(m);
    return mbank_get_prof(*m, local_shard, ms, n);
} LLPF_GUARD(llpf_mbank_get_profile)

// ---- array primitives and device self-tests of the shared primitives (host/primitives.hpp) ----------
int llpf_logsumexp(int32_t device, double* w, double* we, int64_t n, double* ll) LLPF_TRY {
    return prim_logsumexp(device, w, we, n, ll);
} LLPF_GUARD(llpf_logsumexp)
int llpf_resample(int32_t device, int32_t strategy, const double* we, int64_t n, int64_t m, const double* U, int64_t* j) LLPF_TRY {
    return prim_resample(device, strategy, we, n, m, U, j);
} LLPF_GUARD(llpf_resample)
int llpf_resample_uniforms(int32_t strategy, int64_t m, uint64_t seed, uint32_t step, double* u) LLPF_TRY {
    return prim_resample_uniforms(strategy, m, seed, step, u);
} LLPF_GUARD(llpf_resample_uniforms)
int llpf_selftest_math(int32_t device, int32_t which, const double* in, double* out, int64_t n) LLPF_TRY {
    return selftest_math(device, which, in, out, n);
} LLPF_GUARD(llpf_selftest_math)
int llpf_selftest_normals(int32_t device, uint64_t seed, uint32_t step, uint32_t stream, int32_t nd, double* out, int64_t n) LLPF_TRY {
    return selftest_normals(device, seed, step, stream, nd, out, n);
} LLPF_GUARD(llpf_selftest_normals)

}  // extern "C"
