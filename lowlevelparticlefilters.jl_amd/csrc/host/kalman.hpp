// host/kalman.hpp — banks of Kalman filters with constant matrices (llpf_kalman_bank_*; kernel: kernels/kalman.hpp, step:
// shared/llpf_kalman.h).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// Device layout: the constants par [npar][F] and the state [nx + np + 1][F] (x, packed R, the running ll_total of a run), SoA so that
// lane f of a wave reads column f.  A run drives T through the chunked staging pipeline of host/pipe.hpp, counting a step's outputs and
// per-filter inputs; outputs are time-major [T][F][width], per-filter inputs reach the device time-major as well.  The state carries from
// chunk to chunk (and from run to run) in the device buffer, so the prefix of a long run is a short run and run(a) followed by run(b) is
// run(a + b), bit for bit.  A run that asks for ll_total only stages nothing per step.

struct llpf_kalman_bank : BankStream {
    int F = 0, nx = 0, ny = 0, nu = 0;
    int np = 0, npar = 0, nstate = 0;
    DevBuf<double> d_par, d_state;
    DevBuf<double> d_post;            // [T][nx + np][F] the posterior of every step of the last smooth (grow-only: kept between calls)
    std::vector<double> h_init;       // [nstate][F] what reset loads: mean(d0), packed cov(d0), 0
};

// models (+ D [F][ny][nu] or NULL) -> the SoA constants and initial state; every check that needs no device
static int kalman_pack(const llpf_model* models, const double* D, int32_t F, int& nx, int& ny, int& nu, std::vector<double>& par,
                       std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "kalman: models is null");
    if (F < 1) return fail(LLPF_ERR_ARG, "kalman: n_filters must be >= 1");
    nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, "kalman: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    const int np = LLPF_KF_NP(nx), npar = LLPF_KF_NPAR(nx, ny, nu), nstate = nx + np + 1;
    par.assign((size_t)npar * F, 0.0);
    init.assign((size_t)nstate * F, 0.0);
    double S[MAXD * MAXD];
    for (int f = 0; f < F; ++f) {
        const llpf_model& m = models[f];
        const std::string at = "kalman: filter " + std::to_string(f) + ": ";
        if (m.model_id != LLPF_MODEL_LINEAR_GAUSSIAN) return fail(LLPF_ERR_ARG, at + "model_id must be LLPF_MODEL_LINEAR_GAUSSIAN");
        if (m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "dimensions differ from filter 0's");
        const llpf_gaussian* g[3] = {&m.dynamics_density, &m.measurement_density, &m.initial_density};
        const int dims[3] = {nx, ny, nx};
        for (int k = 0; k < 3; ++k) {
            if (g[k]->dim != dims[k]) return fail(LLPF_ERR_ARG, at + "a density's dimension does not match the model");
            if (g[k]->kind != LLPF_COV_SCAL && g[k]->kind != LLPF_COV_DIAG && g[k]->kind != LLPF_COV_FULL)
                return fail(LLPF_ERR_ARG, at + "unknown covariance kind");
        }
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < dims[k]; ++i)
                if (g[k]->mu[i] != 0.0) return fail(LLPF_ERR_ARG, at + "the noise densities must have zero mean");
        GaussD gd;                                // positive definiteness of R2 and P0: the host Cholesky of gauss_prepare
        if (gauss_prepare(&m.measurement_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (gauss_prepare(&m.initial_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
        auto put = [&](int e, double v) { par[(size_t)e * F + f] = v; };
        for (int i = 0; i < nx * nx; ++i) put(LLPF_KF_OFF_A + i, m.A[i]);
        for (int i = 0; i < ny * nx; ++i) put(LLPF_KF_OFF_C(nx) + i, m.C[i]);
        gauss_cov_dense(&m.dynamics_density, S);
        for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) put(LLPF_KF_OFF_R1(nx, ny) + llpf_kf_idx(r, c), S[r * nx + c]);
        gauss_cov_dense(&m.measurement_density, S);
        for (int r = 0; r < ny; ++r) for (int c = 0; c <= r; ++c) put(LLPF_KF_OFF_R2(nx, ny) + llpf_kf_idx(r, c), S[r * ny + c]);
        for (int i = 0; i < nx * nu; ++i) put(LLPF_KF_OFF_B(nx, ny) + i, m.B[i]);
        for (int i = 0; i < ny * nu; ++i) put(LLPF_KF_OFF_D(nx, ny, nu) + i, D ? D[(size_t)f * ny * nu + i] : 0.0);
        gauss_cov_dense(&m.initial_density, S);
        for (int i = 0; i < nx; ++i) init[(size_t)i * F + f] = m.initial_density.mu[i];
        for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) init[(size_t)(nx + llpf_kf_idx(r, c)) * F + f] = S[r * nx + c];
    }
    return LLPF_OK;
}

// the device and the stream of a bank of one-thread-per-filter filters (this file's, and host/ukf.hpp's)
static int kf_open_stream(BankStream& b, int device) {
    b.device = device;
    HIPC(hipSetDevice(device));
    HIPC(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
    return LLPF_OK;
}

static int kalman_create(int32_t device, const llpf_model* models, const double* D, int32_t F, llpf_kalman_bank& b) {
    std::vector<double> par;
    CHK(kalman_pack(models, D, F, b.nx, b.ny, b.nu, par, b.h_init));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(LLPF_ERR_NO_DEVICE, "no HIP device visible; this engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(LLPF_ERR_ARG, "device ordinal out of range");
    test_throw("kalman_create");
    b.F = F;
    b.np = LLPF_KF_NP(b.nx);
    b.npar = LLPF_KF_NPAR(b.nx, b.ny, b.nu);
    b.nstate = b.nx + b.np + 1;
    CHK(kf_open_stream(b, device));
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int kalman_reset(llpf_kalman_bank& b) {
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int kalman_set_models(llpf_kalman_bank& b, const llpf_model* models, const double* D) {
    std::vector<double> par, init;
    int nx = 0, ny = 0, nu = 0;
    CHK(kalman_pack(models, D, b.F, nx, ny, nu, par, init));
    if (nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "kalman: set_models must keep the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    return LLPF_OK;
}

// x [F][nx], R [F][nx][nx] (either may be NULL) of the current state
static int kalman_get_state(llpf_kalman_bank& b, double* x, double* R) {
    std::vector<double> h((size_t)b.nstate * b.F);
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(h.data(), b.d_state, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    const size_t F = (size_t)b.F;
    for (size_t f = 0; f < F; ++f) {
        if (x) for (int i = 0; i < b.nx; ++i) x[f * b.nx + i] = h[i * F + f];
        if (R) for (int r = 0; r < b.nx; ++r) for (int c = 0; c < b.nx; ++c) R[(f * b.nx + r) * b.nx + c] = h[(b.nx + llpf_kf_idx(r, c)) * F + f];
    }
    return LLPF_OK;
}

// the lower triangle of R is taken (R is a covariance: the upper one is not read)
static int kalman_set_state(llpf_kalman_bank& b, const double* x, const double* R) {
    if (!x || !R) return fail(LLPF_ERR_ARG, "kalman: x and R must both be given");
    std::vector<double> h((size_t)b.nstate * b.F, 0.0);
    const size_t F = (size_t)b.F;
    for (size_t f = 0; f < F; ++f) {
        for (int i = 0; i < b.nx; ++i) h[i * F + f] = x[f * b.nx + i];
        for (int r = 0; r < b.nx; ++r) for (int c = 0; c <= r; ++c) h[(b.nx + llpf_kf_idx(r, c)) * F + f] = R[(f * b.nx + r) * b.nx + c];
    }
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// the checks of a run's arguments that need no device (llpf_kalman_bank_run and _smooth)
static int kalman_check_run(const llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter,
                            const llpf_kalman_outputs* out) {
    if (T < 1) return fail(LLPF_ERR_ARG, "kalman: T must be >= 1");
    if (!Y) return fail(LLPF_ERR_ARG, "kalman: Y is null");
    if (b.nu > 0 && !U) return fail(LLPF_ERR_ARG, "kalman: U is null");
    if (per_filter & ~3) return fail(LLPF_ERR_ARG, "kalman: per_filter has bits other than 0 and 1");
    if (out && out->struct_size < sizeof(llpf_kalman_outputs)) return fail(LLPF_ERR_ARG, "kalman: llpf_kalman_outputs.struct_size too small (ABI)");
    return LLPF_OK;
}

static int kalman_forward(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                          const llpf_kalman_outputs* out, double* post);

static int kalman_run(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                      const llpf_kalman_outputs* out) {
    CHK(kalman_check_run(b, U, Y, T, per_filter, out));
    test_throw("kalman_run");
    return kalman_forward(b, U, Y, T, per_filter, ll_total, out, nullptr);
}

// the forward pass of a run (arguments checked); post: null, or the device array [T][nx + np][F] that receives the posterior of every
// step (k_kalman<..., true>).  Everything is allocated before the first launch.
static int kalman_forward(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                          const llpf_kalman_outputs* out, double* post) {
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu;
    const bool upf = nu > 0 && (per_filter & 1), ypf = (per_filter & 2) != 0;
    // the outputs of one step, in staging order: ll, x, xt, R, Rt, e
    double* dst[6] = {out ? out->ll_steps : nullptr, out ? out->x : nullptr, out ? out->xt : nullptr, out ? out->R : nullptr,
                      out ? out->Rt : nullptr, out ? out->e : nullptr};
    const uint64_t width[6] = {1, (uint64_t)nx, (uint64_t)nx, (uint64_t)nx * nx, (uint64_t)nx * nx, (uint64_t)ny};
    uint64_t w = 0;
    std::vector<ChunkOut> outs;
    for (int k = 0; k < 6; ++k) {
        if (dst[k]) w += width[k];
        outs.push_back({dst[k], 1, (size_t)F * width[k]});
    }
    const uint64_t in_w = (upf ? (uint64_t)nu : 0) + (ypf ? (uint64_t)ny : 0);
    uint64_t total = 0, in_total = 0;      // the per-step outputs / per-filter inputs of all filters and steps, in doubles
    if (!doubles_fit({(uint64_t)F, w, (uint64_t)T}, total) || !doubles_fit({(uint64_t)F, in_w, (uint64_t)T}, in_total))
        return fail(LLPF_ERR_ARG, "kalman: the size of the outputs or of the inputs overflows");
    HIPC(hipSetDevice(b.device));
    ChunkPipe pipe(b.stream);
    // (shared inputs and no per-step outputs: nothing per step scales with F, the chunk is CHUNK_STEPS)
    CHK(pipe.open(T, (size_t)F * (w + in_w) * sizeof(double), outs,
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}, {Y, ypf ? (size_t)F : 0, (size_t)ny, true}}));
    for (int64_t c = 0; c < pipe.nchunk; ++c) {
        CHK(pipe.begin(c, c));
        KalmanArgs a{};
        a.par = b.d_par; a.state = b.d_state;
        a.u = pipe.in(0);
        a.y = pipe.in(1);
        double** slot[6] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.e};
        for (int k = 0; k < 6; ++k) *slot[k] = pipe.out(k);
        a.F = F; a.Tc = (int32_t)pipe.tc; a.nu = nu;
        a.u_per = upf ? 1 : 0; a.y_per = ypf ? 1 : 0;
        a.first = c == 0 ? 1 : 0;
        a.par_tstride = 0;
        a.post = post ? post + (size_t)pipe.t0 * (nx + b.np) * F : nullptr;
        HIPC(launch_kalman(nx, ny, a, b.stream));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    if (ll_total)     // the running sum: row nx + np of the state
        HIPC(hipMemcpyAsync(ll_total, b.d_state.p + (size_t)(nx + b.np) * F, sizeof(double) * F, hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// smooth(kf, u, y): the forward pass of a run (the same chunks, outputs and state as kalman_run) that also stores the packed posterior
// of every step on the device (d_post: (nx + np) * 8 bytes per filter-step), then the backward pass k_kalman_smooth over the chunks in
// reverse through a staging pipeline of its own (host/pipe.hpp).  Everything is allocated before the first launch, so a call that cannot
// get its memory leaves the state as it was.  The state after the call is the one kalman_run leaves (the prior of step T and the running
// ll).
static int kalman_smooth(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                         const llpf_kalman_outputs* fwd, const llpf_kalman_smooth_outputs* out) {
    CHK(kalman_check_run(b, U, Y, T, per_filter, fwd));
    if (out && out->struct_size < sizeof(llpf_kalman_smooth_outputs))
        return fail(LLPF_ERR_ARG, "kalman: llpf_kalman_smooth_outputs.struct_size too small (ABI)");
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu, ns = nx + b.np;
    const bool upf = nu > 0 && (per_filter & 1);
    double* dst[2] = {out ? out->xT : nullptr, out ? out->RT : nullptr};
    const uint64_t width[2] = {(uint64_t)nx, (uint64_t)nx * nx};
    const uint64_t w = (dst[0] ? width[0] : 0) + (dst[1] ? width[1] : 0);
    uint64_t post_d = 0, total = 0;
    if (!doubles_fit({(uint64_t)ns, (uint64_t)F, (uint64_t)T}, post_d) || !doubles_fit({(uint64_t)F, w, (uint64_t)T}, total))
        return fail(LLPF_ERR_ARG, "kalman: the size of the stored posterior or of the smoothed outputs overflows");
    test_throw("kalman_smooth");
    if (!w) return kalman_forward(b, U, Y, T, per_filter, ll_total, fwd, nullptr);     // nothing smoothed is asked for: a run
    HIPC(hipSetDevice(b.device));
    CHK(b.d_post.ensure((size_t)post_d));
    ChunkPipe pipe(b.stream);
    double* d_carry = nullptr;
    CHK(pipe.device((size_t)ns * F, d_carry));
    CHK(pipe.open(T, (size_t)F * (w + (upf ? nu : 0)) * sizeof(double), {{dst[0], 1, (size_t)F * width[0]}, {dst[1], 1, (size_t)F * width[1]}},
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}}));
    // the forward pass allocates its own staging before its first launch: no launch has run when it returns an allocation failure
    CHK(kalman_forward(b, U, Y, T, per_filter, ll_total, fwd, b.d_post.p));
    for (int64_t i = 0; i < pipe.nchunk; ++i) {      // backward: launch i runs chunk nchunk - 1 - i
        CHK(pipe.begin(i, pipe.nchunk - 1 - i));
        KalmanSmoothArgs a{};
        a.par = b.d_par;
        a.post = b.d_post.p + (size_t)pipe.t0 * ns * F;
        a.carry = d_carry;
        a.u = pipe.in(0);
        a.xT = pipe.out(0);
        a.RT = pipe.out(1);
        a.F = F; a.Tc = (int32_t)pipe.tc; a.ny = ny; a.nu = nu;
        a.u_per = upf ? 1 : 0;
        a.init = i == 0 ? 1 : 0;
        a.par_tstride = 0;
        HIPC(launch_kalman_smooth(nx, a, b.stream));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
