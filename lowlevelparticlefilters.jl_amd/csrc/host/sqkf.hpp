// host/sqkf.hpp — banks of square-root Kalman filters with constant matrices (llpf_sqkf_bank_*; kernel: kernels/sqkf.hpp, step:
// shared/llpf_sqkf.h).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its state rows and the driver of a run are host/kfbank.hpp's; the pack is host/kalman.hpp's with the three covariances
// factored (llpf_kf_chol, once, here): par holds the packed factors L1, L2 where the Kalman bank holds R1, R2, and the state rows nx ..
// nx + np - 1 hold the packed factor Lr of R.  There is no smoother.

struct llpf_sqkf_bank : KfBank {
    llpf_sqkf_bank() : KfBank("sqkf") {}
};

// the packed triangle in rows row0 .. of the SoA array a [..][F], column f, factored in place; 0: not positive definite
static int sqkf_factor(std::vector<double>& a, int row0, int n, int f, int F) {
    double L[LLPF_KF_NP(LLPF_KF_MAXX)], inv[LLPF_KF_MAXX];
    const int np = LLPF_KF_NP(n);
    for (int i = 0; i < np; ++i) L[i] = a[(size_t)(row0 + i) * F + f];
    const int ok = llpf_kf_chol(n, L, inv);
    for (int i = 0; i < np; ++i) a[(size_t)(row0 + i) * F + f] = L[i];
    return ok;
}

// kalman_pack (its messages under this bank's name), then R1, R2 and cov(d0) of every filter factored
static int sqkf_pack(const llpf_model* models, const double* D, int32_t F, int& nx, int& ny, int& nu, std::vector<double>& par,
                     std::vector<double>& init) {
    const int rc = kalman_pack(models, D, F, nx, ny, nu, par, init);
    if (rc != LLPF_OK) {
        if (g_err.rfind("kalman: ", 0) == 0) g_err = "sqkf: " + g_err.substr(8);
        return rc;
    }
    for (int f = 0; f < F; ++f) {
        const std::string at = "sqkf: filter " + std::to_string(f) + ": ";
        if (!sqkf_factor(par, LLPF_KF_OFF_R1(nx, ny), nx, f, F)) return fail(LLPF_ERR_ARG, at + "R1 (dynamics_density) is not positive definite");
        if (!sqkf_factor(par, LLPF_KF_OFF_R2(nx, ny), ny, f, F)) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (!sqkf_factor(init, nx, nx, f, F)) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
    }
    return LLPF_OK;
}

static int sqkf_create(int32_t device, const llpf_model* models, const double* D, int32_t F, llpf_sqkf_bank& b) {
    std::vector<double> par;
    CHK(sqkf_pack(models, D, F, b.nx, b.ny, b.nu, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_KF_NPAR(b.nx, b.ny, b.nu), "sqkf_create"));
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int sqkf_set_models(llpf_sqkf_bank& b, const llpf_model* models, const double* D) {
    std::vector<double> par, init;
    int nx = 0, ny = 0, nu = 0;
    CHK(sqkf_pack(models, D, b.F, nx, ny, nu, par, init));
    if (nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "sqkf: set_models must keep the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    return LLPF_OK;
}

static int sqkf_run(llpf_sqkf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                    const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    test_throw("sqkf_run");
    const int nx = b.nx, ny = b.ny;
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), nullptr, [&](const KfChunk& c) -> int {
        KalmanArgs a{};
        kf_fill_args(a, b, c);
        HIPC(launch_sqkf(nx, ny, a, b.stream));
        return LLPF_OK;
    });
}

// x [F][nx], R [F][nx][nx] = llpf_sq_cov of the factor, L [F][nx][nx] the dense lower factor (zeros above the diagonal); any may be NULL
// (of any bank whose state rows hold a factor: host/sqekf.hpp's as well)
static int sqkf_get_state(KfBank& b, double* x, double* R, double* L) {
    std::vector<double> h((size_t)b.nstate * b.F);
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(h.data(), b.d_state, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    const size_t F = (size_t)b.F;
    const int nx = b.nx;
    for (size_t f = 0; f < F; ++f) {
        double Lr[LLPF_KF_NP(LLPF_KF_MAXX)], Rp[LLPF_KF_NP(LLPF_KF_MAXX)];
        for (int i = 0; i < b.np; ++i) Lr[i] = h[(nx + i) * F + f];
        llpf_sq_cov(nx, Lr, Rp);
        if (x) for (int i = 0; i < nx; ++i) x[f * nx + i] = h[i * F + f];
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c < nx; ++c) {
                if (R) R[(f * nx + r) * nx + c] = Rp[llpf_kf_idx(r, c)];
                if (L) L[(f * nx + r) * nx + c] = c <= r ? Lr[llpf_kf_idx(r, c)] : 0.0;
            }
    }
    return LLPF_OK;
}

// exactly one of R (its lower triangle, factored with llpf_kf_chol) and L (its lower triangle, as given); the running ll becomes 0
static int sqkf_set_state(KfBank& b, const double* x, const double* R, const double* L) {
    if (!x) return kf_fail(b.who, "x must be given");
    if ((R != nullptr) == (L != nullptr)) return kf_fail(b.who, "exactly one of R and L must be given");
    const double* src = R ? R : L;
    std::vector<double> h((size_t)b.nstate * b.F, 0.0);
    const size_t F = (size_t)b.F;
    const int nx = b.nx;
    for (size_t f = 0; f < F; ++f) {
        for (int i = 0; i < nx; ++i) h[i * F + f] = x[f * nx + i];
        for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) h[(nx + llpf_kf_idx(r, c)) * F + f] = src[(f * nx + r) * nx + c];
        if (R && !sqkf_factor(h, nx, nx, (int)f, b.F))
            return fail(LLPF_ERR_ARG, std::string(b.who) + ": filter " + std::to_string(f) + ": R is not positive definite");
    }
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
