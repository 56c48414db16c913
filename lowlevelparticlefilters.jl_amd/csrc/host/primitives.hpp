// host/primitives.hpp — the array primitives (logsumexp!, resample on the caller's arrays) and the device self-tests of the shared
// primitives.  Part of capi.hip (one translation unit).
// ---- array primitives ------------------------------------------------------------------------------
// a scratch single-filter context with a dummy 1-D model, used for weights-only operations
static int scratch_bank(int32_t device, int64_t n, int strategy, std::unique_ptr<llpf_filter>& out) {
    llpf_config c;
    memset(&c, 0, sizeof(c));
    c.struct_size = sizeof(c);
    c.n_particles = n;
    c.resampling_strategy = strategy;
    c.device = device;
    c.resample_threshold = 0.1;
    c.seed = 0;
    llpf_model& m = c.model;
    m.model_id = LLPF_MODEL_LINEAR_GAUSSIAN;
    m.nx = 1; m.nu = 0; m.ny = 1;
    m.A[0] = 1.0; m.C[0] = 1.0; m.Ts = 1.0; m.supersample = 1;
    llpf_gaussian g;
    memset(&g, 0, sizeof(g));
    g.dim = 1; g.kind = LLPF_COV_SCAL; g.cov[0] = 1.0;
    m.dynamics_density = g; m.measurement_density = g; m.initial_density = g;
    out.reset(new (std::nothrow) llpf_filter());
    if (!out) return fail(LLPF_ERR_ALLOC, "out of host memory");
    const int rc = bank_create(&c, nullptr, 1, out->bank);
    if (rc != LLPF_OK) out.reset();
    return rc;
}

static int prim_logsumexp(int32_t device, double* w, double* we, int64_t n, double* ll) {
    if (!w || n < 1) return fail(LLPF_ERR_ARG, "bad arguments");
    std::unique_ptr<llpf_filter> h;
    CHK(scratch_bank(device, n, LLPF_RESAMPLE_SYSTEMATIC, h));
    Bank& b = h->bank;
    int rc = bank_set_weights(b, w);
    if (rc == LLPF_OK) {
        std::vector<FilterScal> s;
        rc = scal_download(b, s);
        if (rc == LLPF_OK) {
            if (ll) *ll = s[0].ll;
            s[0].norm_pending = 1;     // logsumexp! normalises w in place
            rc = scal_upload(b, s);
        }
        if (rc == LLPF_OK) rc = bank_get_w(b, w, false);
        if (rc == LLPF_OK && we) rc = bank_get_w(b, we, true);
    }
    return rc;
}

static int prim_resample(int32_t device, int32_t strategy, const double* we, int64_t n, int64_t m, const double* U, int64_t* j) {
    if (!we || !U || !j || n < 1 || m < 1) return fail(LLPF_ERR_ARG, "bad arguments");
    if (m > ((int64_t)1 << 30)) return fail(LLPF_ERR_ARG, "m too large");
    std::unique_ptr<llpf_filter> h;
    CHK(scratch_bank(device, n, strategy, h));
    Bank& b = h->bank;
    std::vector<double> stage((size_t)b.Ns, 0.0);
    memcpy(stage.data(), we, sizeof(double) * n);
    HIPC(hipMemcpyAsync(b.d_w, stage.data(), sizeof(double) * b.Ns, hipMemcpyHostToDevice, b.stream));
    const int64_t cap = (m > b.Ns ? m : b.Ns);
    std::vector<int32_t> j32((size_t)cap, 0);
    for (int64_t i = 0; i < m; ++i) j32[i] = (int32_t)j[i];
    DevBuf<int32_t> d_j;
    CHK(d_j.ensure((size_t)cap));
    HIPC(hipMemcpyAsync(d_j, j32.data(), sizeof(int32_t) * cap, hipMemcpyHostToDevice, b.stream));
    const int64_t nU = (strategy == LLPF_RESAMPLE_SYSTEMATIC) ? 1 : m;
    DevBuf<double> d_U;
    CHK(d_U.ensure((size_t)nU));
    HIPC(hipMemcpyAsync(d_U, U, sizeof(double) * nU, hipMemcpyHostToDevice, b.stream));
    std::vector<FilterScal> s;
    CHK(scal_download(b, s));
    s[0].uniform = 0; s[0].anc_ident_s[0] = s[0].anc_ident_s[1] = 0; s[0].status = 0; s[0].do_resample = 1;
    CHK(scal_upload(b, s));
    // ancestors are written relative to a row of stride Ns; the scratch bank has one filter, so row 0
    ResArgs ra{};
    ra.mode = RES_RESAMPLE; ra.M = (int32_t)m; ra.Uexp = d_U; ra.anc_out = d_j; ra.force = 1; ra.src_values = 1;
    HIPC(launch_resample(b.dev(), ra, b.stream));
    CHK(bank_to_host(b, j32.data(), d_j, sizeof(int32_t) * m));
    for (int64_t i = 0; i < m; ++i) j[i] = j32[i];
    return LLPF_OK;
}

// the uniforms a filter's own resampling at `step` draws: pure host code, needs no device
static int prim_resample_uniforms(int32_t strategy, int64_t m, uint64_t seed, uint32_t step, double* u) {
    if (!u) return fail(LLPF_ERR_ARG, "null output");
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (strategy == LLPF_RESAMPLE_SYSTEMATIC) u[0] = llpf_uniform_step(step, LLPF_STREAM_RESAMPLE, k0, k1);
    else for (int64_t i = 0; i < m; ++i) u[i] = llpf_uniform_idx((uint32_t)i, step, LLPF_STREAM_STRATIFY, k0, k1);
    return LLPF_OK;
}

// ---- device self-tests of the shared primitives ---------------------------------------------------
static int selftest_math(int32_t device, int32_t which, const double* in, double* out, int64_t n) {
    CHK(need_device());
    if (!in || !out || n < 1) return fail(LLPF_ERR_ARG, "bad arguments");
    HIPC(hipSetDevice(device));
    DevBuf<double> di, dout;
    CHK(di.ensure((size_t)n));
    CHK(dout.ensure((size_t)n));
    HIPC(hipMemcpy(di, in, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPC(launch_selftest_math(which, di, dout, n, nullptr));
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost));
    return LLPF_OK;
}
static int selftest_normals(int32_t device, uint64_t seed, uint32_t step, uint32_t stream, int32_t nd, double* out, int64_t n) {
    CHK(need_device());
    if (nd < 1 || nd > MAXD) return fail(LLPF_ERR_ARG, "nd out of range");
    if (!out || n < 1) return fail(LLPF_ERR_ARG, "bad arguments");
    HIPC(hipSetDevice(device));
    DevBuf<double> dout;
    CHK(dout.ensure((size_t)n * nd));
    HIPC(launch_selftest_normals((uint32_t)seed, (uint32_t)(seed >> 32), step, stream, nd, dout, n, nullptr));
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(out, dout, sizeof(double) * n * nd, hipMemcpyDeviceToHost));
    return LLPF_OK;
}
