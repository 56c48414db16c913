// host/imm.hpp — banks of interacting-multiple-model filters over Kalman filters with constant matrices, over first-order extended
// Kalman filters or over unscented Kalman filters of one model type (llpf_imm_bank_*; kernels: kernels/imm.hpp, kernels/imm_ekf.hpp,
// kernels/imm_ukf.hpp, step: shared/llpf_imm.h).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank is a KfBank (host/kfbank.hpp) whose columns are lanes: G = 1, 2 or 4 lanes per filter (the smallest G >= M), column f * G + j is
// mode j of filter f, L = F * G columns in all (those of the idle lanes j >= M stay zero).  par is [npar + LLPF_IMM_MAXM][L]: the mode's
// Kalman constants as host/kalman.hpp packs them, then column j of the filter's transition matrix; the state is [nx + np + 2][L]: the
// mode's x, packed R, mu_j and the run's running ll_total (the same number in every lane of a filter).  A run is kf_forward with this
// bank's own outputs.  The combined estimate of get_state is formed on the host from the downloaded state, by the functions of
// shared/llpf_imm.h the kernel forms it with.
// An extended bank (LLPF_IMM_EXTENDED, implied by a model id other than LLPF_MODEL_LINEAR_GAUSSIAN) keeps the columns and the state and
// has, in the place of the Kalman constants, the descriptors ModelD [L] that the model's own functions read and par
// [LLPF_EKF_NPAR + LLPF_IMM_MAXM][L]: R1, R2 packed, then column j of P.  The columns of its idle lanes stay zero as well: k_imm_ekf
// reads mode 0's column in their place.
// An unscented bank (llpf_imm_bank_create_unscented) is the extended bank in everything but two things: its model needs no Jacobian
// members (it passes the checks of llpf_ukf_bank_create instead), and it carries one set of sigma-point weights, which ride in the launch
// arguments of k_imm_ukf.  par is the same R1, R2 block (LLPF_UKF_NPAR is LLPF_EKF_NPAR).

namespace llpf {
#include "../kernels/imm_args.hpp"
// the extended bank's kernel (k_imm_ekf.hip): imm_ekf_prepare compiles the k_imm_ekf of a run-time compiled model at g lanes per filter on
// its first use (0, or -1 with `err` set); launch_imm_ekf runs one chunk of steps
int imm_ekf_prepare(int model_id, int nx, int ny, int g, std::string& err);
hipError_t launch_imm_ekf(int model_id, int nx, int ny, int g, const ModelD* models, const ImmEkfArgs& a, hipStream_t s);
// the unscented bank's kernel (k_imm_ukf.hip), in the same way
int imm_ukf_prepare(int model_id, int nx, int ny, int g, std::string& err);
hipError_t launch_imm_ukf(int model_id, int nx, int ny, int g, const ModelD* models, const ImmUkfArgs& a, hipStream_t s);
}
static int ukf_check_weights(const llpf_ukf_weights* w);      // host/ukf.hpp

// what the modes of a bank are.  The extended and the unscented modes are driven by a model's own functions: they have
// descriptors, a time and no D
enum ImmKind { IMM_KALMAN = 0, IMM_EXTENDED = 1, IMM_UNSCENTED = 2 };

struct llpf_imm_bank : KfBank {
    int M = 0, G = 0, L = 0, interact = 1;
    int kind = IMM_KALMAN, model_id = 0;   // extended, unscented: the modes are such filters of the model `model_id`
    double Ts = 1.0;
    DevBuf<ModelD> d_models;          // extended, unscented: [L] the descriptors the model's own functions read
    DevBuf<double> d_zero;            // extended, unscented: MAXU zeros, the u of a model without inputs
    llpf_ukf_weights w{};             // unscented: the bank's weights
    llpf_imm_bank() : KfBank("imm") {}
};

static int imm_group(int M) { return M <= 1 ? 1 : M == 2 ? 2 : 4; }

// P [M][M] row-stochastic and mu0 [M] a distribution, of one filter (`atf`: its message prefix)
static int imm_check_tables(const double* Pf, const double* mf, int M, const std::string& atf) {
    double smu = 0.0;
    for (int i = 0; i < M; ++i) {
        double srow = 0.0;
        for (int j = 0; j < M; ++j) {
            if (!(Pf[i * M + j] >= 0.0)) return fail(LLPF_ERR_ARG, atf + "row " + std::to_string(i) + " of P has a negative (or NaN) entry");
            srow += Pf[i * M + j];
        }
        if (!(fabs(srow - 1.0) <= 1e-12)) return fail(LLPF_ERR_ARG, atf + "row " + std::to_string(i) + " of P does not sum to 1");
        if (!(mf[i] >= 0.0)) return fail(LLPF_ERR_ARG, atf + "mu0 of mode " + std::to_string(i) + " is negative (or NaN)");
        smu += mf[i];
    }
    if (!(fabs(smu - 1.0) <= 1e-12)) return fail(LLPF_ERR_ARG, atf + "mu0 does not sum to 1");
    return LLPF_OK;
}

// what a mode of a Kalman bank adds to the pack: positive definiteness of R2 and P0, as the Kalman bank checks them, and A, C, B and
// D (Dm [ny][nu], or NULL) as host/kalman.hpp packs them
static int imm_pack_kalman_mode(const llpf_model& m, const std::string& at, const double* Dm, int col, int L, int nx, int ny, int nu,
                                std::vector<double>& par) {
    GaussD gd;
    if (gauss_prepare(&m.measurement_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
    if (gauss_prepare(&m.initial_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
    auto put = [&](int e, double v) { par[(size_t)e * L + col] = v; };
    for (int i = 0; i < nx * nx; ++i) put(LLPF_KF_OFF_A + i, m.A[i]);
    for (int i = 0; i < ny * nx; ++i) put(LLPF_KF_OFF_C(nx) + i, m.C[i]);
    for (int i = 0; i < nx * nu; ++i) put(LLPF_KF_OFF_B(nx, ny) + i, m.B[i]);
    for (int i = 0; i < ny * nu; ++i) put(LLPF_KF_OFF_D(nx, ny, nu) + i, Dm ? Dm[i] : 0.0);
    return LLPF_OK;
}

// models [F][M] (+ D [F][M][ny][nu] or NULL), P [F][M][M], mu0 [F][M] -> the SoA constants and initial state and, of an extended bank,
// the descriptors ModelD [L]; every check that needs no device.  A Kalman bank's modes are linear-Gaussian models; an extended bank's
// are of one model id, which passes the checks of llpf_ekf_bank_create (kf_pack_models on the first model: both Jacobian members, no
// noise / initial / loglik member, not Rao-Blackwellized), an unscented bank's likewise those of llpf_ukf_bank_create (the same without
// the Jacobian members); what a mode adds is imm_pack_kalman_mode or the model's descriptor
static int imm_pack(int kind, const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t F, int32_t M,
                    int& model_id, int& nx, int& ny, int& nu, std::vector<ModelD>& hm, std::vector<double>& par, std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "imm: models is null");
    if (!P || !mu0) return fail(LLPF_ERR_ARG, "imm: P and mu0 must both be given");
    if (F < 1) return fail(LLPF_ERR_ARG, "imm: n_filters must be >= 1");
    if (M < 1 || M > LLPF_IMM_MAXM) return fail(LLPF_ERR_ARG, "imm: n_modes must be in 1..4");
    const bool extended = kind != IMM_KALMAN;      // (below: the modes are driven by a model's own functions)
    if (extended) {
        std::vector<double> par0, init0;
        if (kind == IMM_UNSCENTED) CHK(kf_pack_models("imm", "unscented filter", 0, 0, models, 1, model_id, nx, ny, nu, hm, par0, init0));
        else CHK(kf_pack_models("imm", "extended Kalman filter", LLPF_TRAIT_DYNAMICS_JAC | LLPF_TRAIT_MEASUREMENT_JAC, 0, models, 1, model_id, nx, ny,
                                nu, hm, par0, init0));
    } else {
        model_id = LLPF_MODEL_LINEAR_GAUSSIAN; nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
        if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
            return fail(LLPF_ERR_ARG, "imm: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    }
    const int G = imm_group(M), L = F * G;
    const int np = LLPF_KF_NP(nx), npar = extended ? LLPF_EKF_NPAR(nx, ny) : LLPF_KF_NPAR(nx, ny, nu), nstate = nx + np + 2;
    const int off_r1 = extended ? LLPF_EKF_OFF_R1 : LLPF_KF_OFF_R1(nx, ny), off_r2 = extended ? LLPF_EKF_OFF_R2(nx) : LLPF_KF_OFF_R2(nx, ny);
    hm.assign(extended ? (size_t)L : 0, ModelD{});
    par.assign((size_t)(npar + LLPF_IMM_MAXM) * L, 0.0);
    init.assign((size_t)nstate * L, 0.0);
    for (int f = 0; f < F; ++f) {
        const double* Pf = P + (size_t)f * M * M;
        const double* mf = mu0 + (size_t)f * M;
        CHK(imm_check_tables(Pf, mf, M, "imm: filter " + std::to_string(f) + ": "));
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            const llpf_model& m = models[fj];
            const std::string at = "imm: filter " + std::to_string(f) + ", mode " + std::to_string(j) + ": ";
            const int col = f * G + j;
            if (m.model_id != model_id)
                return fail(LLPF_ERR_ARG, at + (extended ? kind == IMM_UNSCENTED ? "model_id differs from that of filter 0, mode 0: the modes of an unscented bank are one model type"
                                                                              : "model_id differs from that of filter 0, mode 0: the modes of an extended bank are one model type"
                                                         : "model_id must be LLPF_MODEL_LINEAR_GAUSSIAN"));
            if (m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "dimensions differ from those of filter 0, mode 0");
            CHK(kf_pack_filter(m, at, col, L, nx, ny, off_r1, off_r2, par, init));
            if (extended) CHK(kf_model_descriptor(m, at, &hm[(size_t)col]));
            else CHK(imm_pack_kalman_mode(m, at, D ? D + fj * ny * nu : nullptr, col, L, nx, ny, nu, par));
            for (int i = 0; i < M; ++i) par[(size_t)(npar + i) * L + col] = Pf[i * M + j];
            init[(size_t)(nx + np) * L + col] = mf[j];
        }
    }
    return LLPF_OK;
}

static const char* const IMM_NO_D = "imm: D must be NULL when the modes are extended Kalman filters (LLPF_IMM_EXTENDED)";
static const char* const IMM_NO_D_UKF = "imm: D must be NULL when the modes are unscented Kalman filters";

// a bank of the kind b.kind (an unscented one: b.w set), flags checked by the caller
static int imm_create_kind(int32_t device, const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t F, int32_t M,
                           int32_t flags, llpf_imm_bank& b) {
    std::vector<double> par;
    std::vector<ModelD> hm;
    const bool driven = b.kind != IMM_KALMAN;
    if (driven && D) return fail(LLPF_ERR_ARG, b.kind == IMM_UNSCENTED ? IMM_NO_D_UKF : IMM_NO_D);
    CHK(imm_pack(b.kind, models, D, P, mu0, F, M, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    // the kernel of a run-time compiled model, compiled on the first such bank
    auto prepare = [&]() -> int {
        std::string err;
        const int g = imm_group(M);
        const int rc = b.kind == IMM_UNSCENTED ? imm_ukf_prepare(b.model_id, b.nx, b.ny, g, err) : imm_ekf_prepare(b.model_id, b.nx, b.ny, g, err);
        return rc != 0 ? fail(LLPF_ERR_HIP, "imm: " + err) : LLPF_OK;
    };
    // (LLPF_JIT_COMPILE_ONLY=1, the build check on a machine without a GPU as llpf_model_compile knows it: hiprtc cross-compiles the
    // unscented bank's program before a device is asked for; nothing can run.  With a device the call below finds the cache entry.
    // Only this kind: an extended bank under the variable does what it always did, and its tests set it for llpf_model_compile alone)
    const char* co = getenv("LLPF_JIT_COMPILE_ONLY");
    if (b.kind == IMM_UNSCENTED && co && atoi(co)) CHK(prepare());
    CHK(kf_open(b, device, F, driven ? LLPF_EKF_NPAR(b.nx, b.ny) : LLPF_KF_NPAR(b.nx, b.ny, b.nu), "imm_create"));
    if (driven) b.Ts = models[0].Ts;
    b.M = M; b.G = imm_group(M); b.L = F * b.G;
    b.interact = flags & LLPF_IMM_INTERACT;
    b.nstate = b.nx + b.np + 2;
    if (driven) CHK(prepare());
    return kf_upload(b, b.d_models, b.d_zero, hm, par, true);
}

static int imm_create(int32_t device, const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t F, int32_t M,
                      int32_t flags, llpf_imm_bank& b) {
    if (flags & ~(LLPF_IMM_INTERACT | LLPF_IMM_EXTENDED)) return fail(LLPF_ERR_ARG, "imm: flags has bits other than 0 and 1");
    b.kind = ((flags & LLPF_IMM_EXTENDED) || (models && models[0].model_id != LLPF_MODEL_LINEAR_GAUSSIAN)) ? IMM_EXTENDED : IMM_KALMAN;
    return imm_create_kind(device, models, D, P, mu0, F, M, flags, b);
}

// llpf_imm_bank_create_unscented: every mode an unscented Kalman filter, one weight set for the bank
static int imm_create_unscented(int32_t device, const llpf_model* models, const double* P, const double* mu0, int32_t F, int32_t M, int32_t flags,
                                const llpf_ukf_weights* w, llpf_imm_bank& b) {
    if (flags & ~LLPF_IMM_INTERACT) return fail(LLPF_ERR_ARG, "imm: flags of an unscented bank has bits other than 0 (LLPF_IMM_INTERACT)");
    CHK(ukf_check_weights(w));
    b.w = *w;
    b.kind = IMM_UNSCENTED;
    return imm_create_kind(device, models, nullptr, P, mu0, F, M, flags, b);
}

static int imm_set_weights(llpf_imm_bank& b, const llpf_ukf_weights* w) {
    if (b.kind != IMM_UNSCENTED) return fail(LLPF_ERR_ARG, "imm: set_weights needs a bank of unscented modes (llpf_imm_bank_create_unscented)");
    CHK(ukf_check_weights(w));
    b.w = *w;          // the weights ride in launch arguments
    return LLPF_OK;
}

static int imm_set_models(llpf_imm_bank& b, const llpf_model* models, const double* D, const double* P, const double* mu0) {
    std::vector<double> par, init;
    std::vector<ModelD> hm;
    int id = 0, nx = 0, ny = 0, nu = 0;
    const bool driven = b.kind != IMM_KALMAN;
    if (driven && D) return fail(LLPF_ERR_ARG, b.kind == IMM_UNSCENTED ? IMM_NO_D_UKF : IMM_NO_D);
    CHK(imm_pack(b.kind, models, D, P, mu0, b.F, b.M, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu)
        return fail(LLPF_ERR_ARG, driven ? "imm: set_models must keep the model id and the dimensions of the bank"
                                             : "imm: set_models must keep the dimensions of the bank");
    CHK(kf_upload(b, b.d_models, b.d_zero, hm, par, false));
    b.h_init.swap(init);
    if (driven) b.Ts = models[0].Ts;
    return LLPF_OK;
}

// t_index0 (the C ABI checks it before it looks at the handle): step t of an extended or unscented bank runs at tau = (t_index0 + t) * Ts; a Kalman
// bank ignores it
static int imm_check_time(double t_index0) {
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "imm: t_index0 must be finite");
    return LLPF_OK;
}

// T steps of every filter from the current state: kf_forward with this bank's seven outputs and k_imm, k_imm_ekf or k_imm_ukf.  ll_total is row
// nx + np + 1 of the state, the same number in every lane of a filter
static int imm_run(llpf_imm_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                   const llpf_imm_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out, "llpf_imm_outputs"));
    CHK(imm_check_time(t_index0));
    test_throw("imm_run");
    const uint64_t nx = (uint64_t)b.nx, M = (uint64_t)b.M;
    const llpf_imm_outputs none{};
    if (!out) out = &none;
    const KfOutputs o{7, {out->ll_steps, out->x, out->xt, out->R, out->Rt, out->mu, out->ll_modes}, {1, nx, nx, nx * nx, nx * nx, M, M},
                      ll_total, b.nx + b.np + 1, b.G};
    return kf_forward(b, U, Y, T, per_filter, o, nullptr, [&](const KfChunk& c) -> int {
        ImmBaseArgs a{};
        a.par = b.d_par; a.state = b.d_state;
        a.u = c.u;
        a.y = c.y;
        double** slot[7] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.mu, &a.ll_modes};
        for (int k = 0; k < 7; ++k) *slot[k] = c.out[k];
        a.F = b.F; a.Tc = c.tc; a.nu = b.nu; a.M = b.M;
        a.u_per = c.upf; a.y_per = c.ypf;
        a.first = c.first;
        a.interact = b.interact;
        const ImmEkfArgs ea{a, b.d_zero, c.t0, t_index0, b.Ts};
        if (b.kind == IMM_UNSCENTED)
            HIPC(launch_imm_ukf(b.model_id, b.nx, b.ny, b.G, b.d_models, ImmUkfArgs{ea, b.w.gamma, b.w.wm0, b.w.wc0, b.w.wi}, b.stream));
        else if (b.kind == IMM_EXTENDED) HIPC(launch_imm_ekf(b.model_id, b.nx, b.ny, b.G, b.d_models, ea, b.stream));
        else HIPC(launch_imm(b.nx, b.ny, b.G, ImmArgs{a, 0}, b.stream));
        return LLPF_OK;
    });
}

// the combined x [F][nx], R [F][nx][nx], and mu [F][M], the modes' xm [F][M][nx], Rm [F][M][nx][nx] of the current state (each may be NULL)
static int imm_get_state(llpf_imm_bank& b, double* x, double* R, double* mu, double* xm, double* Rm) {
    std::vector<double> h((size_t)b.nstate * b.L);
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(h.data(), b.d_state, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    const size_t L = (size_t)b.L;
    const int nx = b.nx, np = b.np, M = b.M;
    for (int f = 0; f < b.F; ++f) {
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][LLPF_KF_NP(LLPF_KF_MAXX)], ms[LLPF_IMM_MAXM];
        for (int j = 0; j < M; ++j) {
            const size_t col = (size_t)f * b.G + j, fj = (size_t)f * M + j;
            for (int i = 0; i < nx; ++i) xs[j][i] = h[i * L + col];
            for (int i = 0; i < np; ++i) Rs[j][i] = h[(nx + i) * L + col];
            ms[j] = h[(size_t)(nx + np) * L + col];
            if (mu) mu[fj] = ms[j];
            if (xm) for (int i = 0; i < nx; ++i) xm[fj * nx + i] = xs[j][i];
            if (Rm) for (int r = 0; r < nx; ++r) for (int c = 0; c < nx; ++c) Rm[(fj * nx + r) * nx + c] = Rs[j][llpf_kf_idx(r, c)];
        }
        if (!x && !R) continue;
        double xc[LLPF_KF_MAXX] = {0.0}, Rc[LLPF_KF_NP(LLPF_KF_MAXX)] = {0.0};
        for (int j = 0; j < M; ++j) llpf_imm_mean_add(nx, ms[j], xs[j], xc);
        for (int j = 0; j < M; ++j) llpf_imm_cov_add(nx, ms[j], xs[j], Rs[j], xc, Rc);
        if (x) for (int i = 0; i < nx; ++i) x[(size_t)f * nx + i] = xc[i];
        if (R) for (int r = 0; r < nx; ++r) for (int c = 0; c < nx; ++c) R[((size_t)f * nx + r) * nx + c] = Rc[llpf_kf_idx(r, c)];
    }
    return LLPF_OK;
}

// mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx] (the lower triangles are taken); the running ll_total is zeroed
static int imm_set_state(llpf_imm_bank& b, const double* mu, const double* xm, const double* Rm) {
    if (!mu || !xm || !Rm) return kf_fail(b.who, "mu, x and R of the modes must all be given");
    std::vector<double> h((size_t)b.nstate * b.L, 0.0);
    const size_t L = (size_t)b.L;
    const int nx = b.nx, np = b.np, M = b.M;
    for (int f = 0; f < b.F; ++f)
        for (int j = 0; j < M; ++j) {
            const size_t col = (size_t)f * b.G + j, fj = (size_t)f * M + j;
            for (int i = 0; i < nx; ++i) h[i * L + col] = xm[fj * nx + i];
            for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) h[(nx + llpf_kf_idx(r, c)) * L + col] = Rm[(fj * nx + r) * nx + c];
            h[(size_t)(nx + np) * L + col] = mu[fj];
        }
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
