// host/access.hpp — accessors and set_weights.  Part of capi.hip (one translation unit).
// ---- accessors ----------------------------------------------------------------------------------
static int bank_get_particles(Bank& b, double* dst) {
    CHK(use_device(b));
    BankDev d = b.devp();
    HIPC(launch_soa2aos(d, b.d_x[b.cur], b.d_tmp, b.stream));
    return bank_to_host(b, dst, b.d_tmp, sizeof(double) * (size_t)b.F * b.N * b.nxp);
}
static int bank_get_w(Bank& b, double* dst, bool expw) {
    CHK(use_device(b));
    if (expw && b.we_is_lambda) {     // after an aux predict! the reference's `we` holds lambda (src/filtering.jl:200-203)
        HIPC(hipMemcpy2DAsync(dst, sizeof(double) * b.N, b.d_lam, sizeof(double) * b.Ns, sizeof(double) * b.N, b.F,
                              hipMemcpyDeviceToHost, b.stream));
        HIPC(hipStreamSynchronize(b.stream));
        return LLPF_OK;
    }
    BankDev d = b.dev();
    HIPC(launch_materialize(d, expw ? nullptr : b.d_tmp, expw ? b.d_tmp : nullptr, b.stream));
    return bank_to_host(b, dst, b.d_tmp, sizeof(double) * (size_t)b.F * b.N);
}
// (single filter, as the accessors below)
static int bank_get_ancestors(Bank& b, int64_t* dst) {
    CHK(use_device(b));
    HIPC(launch_anc64(b.dev(), reinterpret_cast<int64_t*>(b.d_tmp), b.stream));
    return bank_to_host(b, dst, b.d_tmp, sizeof(int64_t) * b.N);
}
static int bank_get_bins(Bank& b, double* dst) {
    if (!dst) return fail(LLPF_ERR_ARG, "null output");
    if (b.cfg.resampling_strategy == LLPF_RESAMPLE_RESIDUAL)   // the reference leaves the bins of the RESIDUAL weights there (src/resample.jl:98-104)
        return fail(LLPF_ERR_ARG, "state(pf).bins is not provided for residual resampling");
    CHK(use_device(b));
    BankDev d = b.dev();
    ResArgs ra{};
    ra.mode = RES_RESAMPLE; ra.step = rel_step(b); ra.M = (int32_t)b.N; ra.anc_out = b.d_anc;
    ra.parity = (b.parity + ACC_NSLOT - 1) % ACC_NSLOT;
    ra.bins_out = b.d_tmp; ra.only_bins = 1; ra.force = 1;
    HIPC(launch_resample(d, ra, b.stream));
    return bank_to_host(b, dst, b.d_tmp, sizeof(double) * b.N);
}
static int bank_set_particles(Bank& b, const double* src) {
    CHK(use_device(b));
    HIPC(hipMemcpyAsync(b.d_tmp, src, sizeof(double) * b.N * b.nxp, hipMemcpyHostToDevice, b.stream));
    HIPC(launch_aos2soa(b.devp(), b.d_tmp, b.d_x[b.cur], b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// the scalars of filter 0; decide: with effective_particles and shouldresample of the stored state
static int bank_scal0(Bank& b, FilterScal* out, bool decide) {
    CHK(use_device(b));
    if (decide) HIPC(launch_ess(b.dev(), b.stream));   // sum e^2 may have been skipped by the hot loop (threshold 1)
    std::vector<FilterScal> h;
    CHK(scal_download(b, h));
    *out = h[0];
    if (decide && !out->status) {   // shouldresample on the stored state (reference src/resample.jl:5-10)
        if (out->uniform) {
            const double wev = 1.0 / (double)b.N;
            out->ess = 1.0 / ((double)b.N * (wev * wev));
        }
        const double thr = b.cfg.resample_threshold;
        out->do_resample = (thr == 1.0) ? 1 : (out->ess < (double)b.N * thr ? 1 : 0);
    }
    return LLPF_OK;
}

static int bank_weighted_mean(Bank& b, double* xh) {
    CHK(use_device(b));
    CHK(bank_wmean(b, b.d_tmp));
    return bank_to_host(b, xh, b.d_tmp, sizeof(double) * b.nxp);
}
static int bank_weighted_cov(Bank& b, double* cov) {
    if (!cov) return fail(LLPF_ERR_ARG, "null output");
    if (is_rbfull(b)) return fail(LLPF_ERR_ARG, "weighted_cov is not provided for LLPF_MODEL_RB_BILINEAR (take it from the particles)");
    CHK(use_device(b));
    // d_tmp: the mean in [0, MAXD), the covariance in [MAXD, MAXD + nx * nx) — bank_carve sizes it for MAXD + MAXD * MAXD whatever N
    CHK(bank_wmean(b, b.d_tmp));
    HIPC(launch_wcov(b.dev(), b.d_tmp, b.d_tmp + MAXD, b.stream));
    return bank_to_host(b, cov, b.d_tmp + MAXD, sizeof(double) * b.nx * b.nx);
}
static int bank_weighted_quantile(Bank& b, const double* q, int32_t nq, double* out) {
    if (!q || !out) return fail(LLPF_ERR_ARG, "null pointer");
    if (nq < 1 || nq > 1024) return fail(LLPF_ERR_ARG, "llpf_weighted_quantile: 1 <= nq <= 1024");
    for (int i = 0; i < nq; ++i) if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(LLPF_ERR_ARG, "llpf_weighted_quantile: a probability outside [0, 1]");
    if (is_rbfull(b)) return fail(LLPF_ERR_ARG, "weighted_quantile is not provided for LLPF_MODEL_RB_BILINEAR (take it from the particles)");
    if (b.we_is_lambda) return fail(LLPF_ERR_ARG, "weighted_quantile between the halves of an auxiliary predict!: expweights(pf) holds lambda there");
    CHK(use_device(b));
    BankDev d = b.dev();
    CHK(ensure_wq(b, q, nq));
    HIPC(hipStreamSynchronize(b.stream));                                     // q is the caller's (pageable) memory
    HIPC(launch_materialize(d, nullptr, b.d_wq_we, b.stream));               // we = expweights(pf), [N]
    CHK(b.d_xquant.ensure((size_t)nq * b.nx));
    HIPC(launch_wquantile(d.xcur, b.Ns, b.nx, b.d_wq_we, b.N, b.d_wq_p, nq, b.d_xquant, b.nx, 1, b.d_wq, b.stream));      // [nq][nx]
    return bank_to_host(b, out, b.d_xquant, sizeof(double) * (size_t)nq * b.nx);
}

// x[1].R of an RBPF: the covariance of the linear substate, shared by all particles and kept on the host (host/rbkf.hpp)
static int bank_rb_covariance(Bank& b, double* R) {
    if (!is_rb(b)) return fail(LLPF_ERR_ARG, "not a Rao-Blackwellized filter");
    if (!R) return fail(LLPF_ERR_ARG, "null output");
    const int nl = b.nx - b.cfg.model.nxn;
    for (int i = 0; i < nl * nl; ++i) R[i] = b.rb[0].R[i];
    return LLPF_OK;
}
// the per-particle Kalman state of LLPF_MODEL_RB_BILINEAR: the rows of the plane below xn are xl and the packed R
static int bank_rb_linear_state(Bank& b, double* xl, double* R) {
    if (!is_rbfull(b)) return fail(LLPF_ERR_ARG, "not a filter with per-particle covariance (LLPF_MODEL_RB_BILINEAR)");
    CHK(use_device(b));
    const int nn = b.nx, nl = b.cfg.model.rb.nxl, np = LLPF_RBF_NP(nl);
    std::vector<double> rows((size_t)(nl + np) * b.Ns);
    CHK(bank_to_host(b, rows.data(), b.d_x[b.cur] + (size_t)nn * b.Ns, sizeof(double) * rows.size()));
    for (int64_t i = 0; i < b.N; ++i) {
        if (xl) for (int d = 0; d < nl; ++d) xl[i * nl + d] = rows[(size_t)d * b.Ns + i];
        if (R) for (int r = 0; r < nl; ++r) for (int c = 0; c < nl; ++c)
            R[(i * nl + r) * nl + c] = rows[(size_t)(nl + llpf_rbf_idx(r, c)) * b.Ns + i];
    }
    return LLPF_OK;
}

static int bank_set_weights(Bank& b, const double* w) {
    CHK(use_device(b));
    b.aux_pending = false; b.we_is_lambda = false;
    std::vector<double> stage((size_t)b.F * b.Ns, -INFINITY);
    for (int f = 0; f < b.F; ++f) memcpy(stage.data() + (size_t)f * b.Ns, w + (size_t)f * b.N, sizeof(double) * b.N);
    HIPC(hipMemcpyAsync(b.d_w, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    std::vector<FilterScal> h;
    CHK(scal_download(b, h));
    for (auto& s : h) { s.uniform = 0; s.norm_pending = 0; s.status = 0; }
    CHK(scal_upload(b, h));
    CHK(bank_zero_acc(b));
    BankDev d = b.dev();
    HIPC(launch_max(d, b.parity, b.stream));
    HIPC(launch_norm(d, b.parity, 0, 1, rel_step(b), 0, 0, 0, b.stream));
    ResArgs ra{};
    ra.mode = RES_FINALIZE; ra.parity = b.parity; ra.M = (int32_t)b.N; ra.keep_norm = 1; ra.fast_head = 0;
    HIPC(launch_resample(d, ra, b.stream));
    b.parity = (b.parity + 1) % ACC_NSLOT;
    CHK(scal_download(b, h));
    return check_status(b, h);
}
