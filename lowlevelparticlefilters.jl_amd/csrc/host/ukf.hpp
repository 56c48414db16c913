// host/ukf.hpp — banks of unscented Kalman filters (llpf_ukf_bank_*; kernel: kernels/ukf.hpp, step: shared/llpf_ukf.h).  Part of
// capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// Device layout: the model descriptors ModelD[F] as a bank of particle filters keeps them (the model's own parameters), the covariances
// par [np(nx) + np(ny)][F] (R1, R2 packed, from the llpf_model covariances as given — GaussD keeps a factor, not the covariance) and
// the state [nx + np + 1][F] (x, packed R, the running ll_total of a run), SoA as the Kalman bank's.  A run drives T through the chunked
// staging pipeline of host/pipe.hpp exactly as kalman_forward does; the state carries from chunk to chunk (and from run to run) in the
// device buffer, so run(a) followed by run(b) is run(a + b), bit for bit.  A run that asks for ll_total only stages nothing per step.
// A smooth (ukf_smooth) is that run with the posterior of every step kept on the device, and k_ukf_smooth over the chunks in reverse.

struct llpf_ukf_bank : BankStream {
    int F = 0, nx = 0, ny = 0, nu = 0;
    int np = 0, npar = 0, nstate = 0;
    int model_id = 0;
    double Ts = 1.0;
    llpf_ukf_weights w{};
    DevBuf<ModelD> d_models;
    DevBuf<double> d_par, d_state, d_zero;
    DevBuf<double> d_post;            // [T][nx + np][F] the posterior of every step of the last smooth (grow-only: kept between calls)
    std::vector<double> h_init;       // [nstate][F] what reset loads: mean(d0), packed cov(d0), 0
};

// every check of the weights that needs no device
static int ukf_check_weights(const llpf_ukf_weights* w) {
    if (!w) return fail(LLPF_ERR_ARG, "ukf: weights is null");
    if (w->struct_size < sizeof(llpf_ukf_weights)) return fail(LLPF_ERR_ARG, "ukf: llpf_ukf_weights.struct_size too small (ABI)");
    if (!std::isfinite(w->gamma) || !std::isfinite(w->wm0) || !std::isfinite(w->wc0) || !std::isfinite(w->wi))
        return fail(LLPF_ERR_ARG, "ukf: the weights must be finite");
    if (!(w->gamma > 0.0) || !(w->wi > 0.0)) return fail(LLPF_ERR_ARG, "ukf: gamma and wi must be > 0");
    return LLPF_OK;
}

// models -> the descriptors, the SoA covariances and the initial state; every check that needs no device
static int ukf_pack(const llpf_model* models, int32_t F, int& model_id, int& nx, int& ny, int& nu, std::vector<ModelD>& hm,
                    std::vector<double>& par, std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "ukf: models is null");
    if (F < 1) return fail(LLPF_ERR_ARG, "ukf: n_filters must be >= 1");
    model_id = models[0].model_id; nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (model_id == LLPF_MODEL_RB_LINEAR || model_id == LLPF_MODEL_RB_BILINEAR)
        return fail(LLPF_ERR_ARG, "ukf: the Rao-Blackwellized models (LLPF_MODEL_RB_LINEAR, LLPF_MODEL_RB_BILINEAR) have no unscented filter");
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, "ukf: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2 || nu != 2) return fail(LLPF_ERR_ARG, "ukf: the quad-tank has 4 states, 2 outputs and 2 inputs");
    } else if (model_id >= LLPF_MODEL_USER_BASE) {
        std::string src;
        int sx = 0, sy = 0;
        if (!jit_model_source(model_id, src, sx, sy)) return fail(LLPF_ERR_ARG, "ukf: unknown model id " + std::to_string(model_id));
        if (sx != nx || sy != ny) return fail(LLPF_ERR_ARG, "ukf: nx, ny differ from the dimensions the model was compiled for");
        const int traits = jit_model_traits(model_id);
        if (traits & LLPF_TRAIT_LOGLIK) return fail(LLPF_ERR_ARG, "ukf: the model has a likelihood of its own (loglik): there is no Gaussian R2");
        if (traits & LLPF_TRAIT_NOISE) return fail(LLPF_ERR_ARG, "ukf: the model forms its own noise (noise): only additive noise is supported");
        if (traits & LLPF_TRAIT_INITIAL) return fail(LLPF_ERR_ARG, "ukf: the model has an initial density of its own (initial): d0 must be Gaussian");
    } else if (model_id != LLPF_MODEL_LINEAR_GAUSSIAN) {
        return fail(LLPF_ERR_ARG, "ukf: unknown model id " + std::to_string(model_id));
    }
    const int np = LLPF_KF_NP(nx), npar = LLPF_UKF_NPAR(nx, ny), nstate = nx + np + 1;
    hm.resize((size_t)F);
    par.assign((size_t)npar * F, 0.0);
    init.assign((size_t)nstate * F, 0.0);
    double S[MAXD * MAXD];
    for (int f = 0; f < F; ++f) {
        const llpf_model& m = models[f];
        const std::string at = "ukf: filter " + std::to_string(f) + ": ";
        if (m.model_id != model_id || m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "model id or dimensions differ from filter 0's");
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
        const int rc = model_prepare(&m, &hm[(size_t)f]);      // the descriptor the model's own methods read; positive definiteness of R1, R2, cov(d0)
        if (rc == -1) return fail(LLPF_ERR_ARG, at + "R1 (dynamics_density) is not positive definite");
        if (rc == -2) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (rc == -3) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
        if (rc) return fail(LLPF_ERR_ARG, at + "invalid model descriptor, code " + std::to_string(rc));
        auto put = [&](int e, double v) { par[(size_t)e * F + f] = v; };
        gauss_cov_dense(&m.dynamics_density, S);
        for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) put(LLPF_UKF_OFF_R1 + llpf_kf_idx(r, c), S[r * nx + c]);
        gauss_cov_dense(&m.measurement_density, S);
        for (int r = 0; r < ny; ++r) for (int c = 0; c <= r; ++c) put(LLPF_UKF_OFF_R2(nx) + llpf_kf_idx(r, c), S[r * ny + c]);
        gauss_cov_dense(&m.initial_density, S);
        for (int i = 0; i < nx; ++i) init[(size_t)i * F + f] = m.initial_density.mu[i];
        for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) init[(size_t)(nx + llpf_kf_idx(r, c)) * F + f] = S[r * nx + c];
    }
    return LLPF_OK;
}

static int ukf_create(int32_t device, const llpf_model* models, int32_t F, const llpf_ukf_weights* w, llpf_ukf_bank& b) {
    std::vector<ModelD> hm;
    std::vector<double> par;
    CHK(ukf_check_weights(w));
    CHK(ukf_pack(models, F, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(LLPF_ERR_NO_DEVICE, "no HIP device visible; this engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(LLPF_ERR_ARG, "device ordinal out of range");
    test_throw("ukf_create");
    b.F = F;
    b.np = LLPF_KF_NP(b.nx);
    b.npar = LLPF_UKF_NPAR(b.nx, b.ny);
    b.nstate = b.nx + b.np + 1;
    b.Ts = models[0].Ts;
    b.w = *w;
    CHK(kf_open_stream(b, device));
    {
        std::string err;      // a run-time compiled model's k_ukf, on the first bank of that model
        if (ukf_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, "ukf: " + err);
    }
    CHK(b.d_models.ensure(hm.size()));
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    CHK(b.d_zero.ensure(MAXU));
    HIPC(hipMemsetAsync(b.d_zero, 0, sizeof(double) * MAXU, b.stream));
    HIPC(hipMemcpyAsync(b.d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int ukf_reset(llpf_ukf_bank& b) {
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int ukf_set_models(llpf_ukf_bank& b, const llpf_model* models) {
    std::vector<ModelD> hm;
    std::vector<double> par, init;
    int id = 0, nx = 0, ny = 0, nu = 0;
    CHK(ukf_pack(models, b.F, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "ukf: set_models must keep the model id and the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    b.Ts = models[0].Ts;
    return LLPF_OK;
}

static int ukf_set_weights(llpf_ukf_bank& b, const llpf_ukf_weights* w) {
    CHK(ukf_check_weights(w));
    b.w = *w;          // the weights ride in launch arguments
    return LLPF_OK;
}

// x [F][nx], R [F][nx][nx] (either may be NULL) of the current state
static int ukf_get_state(llpf_ukf_bank& b, double* x, double* R) {
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
static int ukf_set_state(llpf_ukf_bank& b, const double* x, const double* R) {
    if (!x || !R) return fail(LLPF_ERR_ARG, "ukf: x and R must both be given");
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

// the checks of a run's arguments that need no device (llpf_ukf_bank_run and _smooth)
static int ukf_check_run(const llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0,
                         const llpf_kalman_outputs* out) {
    if (T < 1) return fail(LLPF_ERR_ARG, "ukf: T must be >= 1");
    if (!Y) return fail(LLPF_ERR_ARG, "ukf: Y is null");
    if (b.nu > 0 && !U) return fail(LLPF_ERR_ARG, "ukf: U is null");
    if (per_filter & ~3) return fail(LLPF_ERR_ARG, "ukf: per_filter has bits other than 0 and 1");
    if (out && out->struct_size < sizeof(llpf_kalman_outputs)) return fail(LLPF_ERR_ARG, "ukf: llpf_kalman_outputs.struct_size too small (ABI)");
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "ukf: t_index0 must be finite");
    return LLPF_OK;
}

static int ukf_forward(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                       const llpf_kalman_outputs* out, double* post);

// T steps of every filter from the current state
static int ukf_run(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                   const llpf_kalman_outputs* out) {
    CHK(ukf_check_run(b, U, Y, T, per_filter, t_index0, out));
    test_throw("ukf_run");
    return ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, out, nullptr);
}

// the forward pass of a run (arguments checked); post: null, or the device array [T][nx + np][F] that receives the posterior of every
// step (k_ukf<..., true>).  Everything is allocated before the first launch.
static int ukf_forward(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
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
    uint64_t total = 0, in_total = 0;
    if (!doubles_fit({(uint64_t)F, w, (uint64_t)T}, total) || !doubles_fit({(uint64_t)F, in_w, (uint64_t)T}, in_total))
        return fail(LLPF_ERR_ARG, "ukf: the size of the outputs or of the inputs overflows");
    HIPC(hipSetDevice(b.device));
    ChunkPipe pipe(b.stream);
    CHK(pipe.open(T, (size_t)F * (w + in_w) * sizeof(double), outs,
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}, {Y, ypf ? (size_t)F : 0, (size_t)ny, true}}));
    for (int64_t c = 0; c < pipe.nchunk; ++c) {
        CHK(pipe.begin(c, c));
        UkfArgs a{};
        a.par = b.d_par; a.state = b.d_state; a.zero_u = b.d_zero;
        a.u = pipe.in(0);
        a.y = pipe.in(1);
        double** slot[6] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.e};
        for (int k = 0; k < 6; ++k) *slot[k] = pipe.out(k);
        a.F = F; a.t0 = pipe.t0; a.Tc = (int32_t)pipe.tc; a.nu = nu;
        a.u_per = upf ? 1 : 0; a.y_per = ypf ? 1 : 0;
        a.first = c == 0 ? 1 : 0;
        a.t_index0 = t_index0; a.Ts = b.Ts;
        a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
        a.post = post ? post + (size_t)pipe.t0 * (nx + b.np) * F : nullptr;
        HIPC(launch_ukf(b.model_id, nx, ny, b.d_models, a, b.stream));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    if (ll_total)     // the running sum: row nx + np of the state
        HIPC(hipMemcpyAsync(ll_total, b.d_state.p + (size_t)(nx + b.np) * F, sizeof(double) * F, hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// smooth(ukf, u, y): the forward pass of a run (the same chunks, outputs and state as ukf_run) that also stores the packed posterior of
// every step on the device (d_post: (nx + np) * 8 bytes per filter-step), then the backward pass k_ukf_smooth over the chunks in reverse
// through a staging pipeline of its own (host/pipe.hpp) — kalman_smooth, with the model's dynamics in the place of A.  A run-time
// compiled model's k_ukf_smooth is compiled first; everything is allocated before the first launch, so a call that cannot get its memory
// leaves the state as it was.  The state after the call is the one ukf_run leaves (the prior of step T and the running ll).
static int ukf_smooth(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                      const llpf_kalman_outputs* fwd, const llpf_kalman_smooth_outputs* out) {
    CHK(ukf_check_run(b, U, Y, T, per_filter, t_index0, fwd));
    if (out && out->struct_size < sizeof(llpf_kalman_smooth_outputs))
        return fail(LLPF_ERR_ARG, "ukf: llpf_kalman_smooth_outputs.struct_size too small (ABI)");
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu, ns = nx + b.np;
    const bool upf = nu > 0 && (per_filter & 1);
    double* dst[2] = {out ? out->xT : nullptr, out ? out->RT : nullptr};
    const uint64_t width[2] = {(uint64_t)nx, (uint64_t)nx * nx};
    const uint64_t w = (dst[0] ? width[0] : 0) + (dst[1] ? width[1] : 0);
    uint64_t post_d = 0, total = 0;
    if (!doubles_fit({(uint64_t)ns, (uint64_t)F, (uint64_t)T}, post_d) || !doubles_fit({(uint64_t)F, w, (uint64_t)T}, total))
        return fail(LLPF_ERR_ARG, "ukf: the size of the stored posterior or of the smoothed outputs overflows");
    test_throw("ukf_smooth");
    if (!w) return ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, fwd, nullptr);     // nothing smoothed is asked for: a run
    HIPC(hipSetDevice(b.device));
    {
        std::string err;      // a run-time compiled model's k_ukf_smooth and k_ukf<..., true>, on the first smooth of that model
        if (ukf_smooth_prepare(b.model_id, nx, ny, err) != 0) return fail(LLPF_ERR_HIP, "ukf: " + err);
    }
    CHK(b.d_post.ensure((size_t)post_d));
    ChunkPipe pipe(b.stream);
    double* d_carry = nullptr;
    CHK(pipe.device((size_t)ns * F, d_carry));
    CHK(pipe.open(T, (size_t)F * (w + (upf ? nu : 0)) * sizeof(double), {{dst[0], 1, (size_t)F * width[0]}, {dst[1], 1, (size_t)F * width[1]}},
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}}));
    // the forward pass allocates its own staging before its first launch: no launch has run when it returns an allocation failure
    CHK(ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, fwd, b.d_post.p));
    for (int64_t i = 0; i < pipe.nchunk; ++i) {      // backward: launch i runs chunk nchunk - 1 - i
        CHK(pipe.begin(i, pipe.nchunk - 1 - i));
        UkfSmoothArgs a{};
        a.par = b.d_par;
        a.post = b.d_post.p + (size_t)pipe.t0 * ns * F;
        a.carry = d_carry;
        a.u = pipe.in(0);
        a.zero_u = b.d_zero;
        a.xT = pipe.out(0);
        a.RT = pipe.out(1);
        a.F = F; a.t0 = pipe.t0; a.Tc = (int32_t)pipe.tc; a.nu = nu;
        a.u_per = upf ? 1 : 0;
        a.init = i == 0 ? 1 : 0;
        a.t_index0 = t_index0; a.Ts = b.Ts;
        a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
        HIPC(launch_ukf_smooth(b.model_id, nx, ny, b.d_models, a, b.stream));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
