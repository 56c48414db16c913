// host/kfbank.hpp — what the banks of Kalman filters share (host/kalman.hpp, host/sqkf.hpp, host/imm.hpp, host/ukf.hpp, host/ekf.hpp,
// host/enkf.hpp): the bank, its state, the checks of a run's arguments and the drivers of the forward and the backward pass; for the
// model-driven banks also their models (KfModelBank).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// Device layout: the constants par [npar][F] (each bank's own rows) and the state [nx + np + 1][F] (x, packed R, the running ll_total of a
// run), SoA so that lane f of a wave reads column f.  A run drives T through the chunked staging pipeline of host/pipe.hpp, counting a
// step's outputs and per-filter inputs; outputs are time-major [T][F][width], per-filter inputs reach the device time-major as well.  The
// state carries from chunk to chunk (and from run to run) in the device buffer, so the prefix of a long run is a short run and run(a)
// followed by run(b) is run(a + b), bit for bit.  A run that asks for ll_total only stages nothing per step.
// Nothing here knows which bank it serves: a bank gives its name (the prefix of its messages), its fault-injection sites, the list of
// its per-step outputs (KfOutputs) and, per chunk, a launcher that fills its kernel's own argument struct from a KfChunk / KfSmoothChunk.

struct KfBank : BankStream {
    const char* who;                  // "kalman" / "ukf": the prefix of every message
    int F = 0, nx = 0, ny = 0, nu = 0;
    int np = 0, npar = 0, nstate = 0;
    DevBuf<double> d_par, d_state;
    DevBuf<double> d_post;            // [T][nx + np][F] the posterior of every step of the last smooth (grow-only: kept between calls)
    std::vector<double> h_init;       // [nstate][F] what reset loads: mean(d0), packed cov(d0), 0
    explicit KfBank(const char* who_) : who(who_) {}
};

static int kf_fail(const char* who, const char* msg) { return fail(LLPF_ERR_ARG, std::string(who) + ": " + msg); }

// the part of a pack that every filter of either bank needs: the checks of the three densities (`at`: the filter's message prefix), R1
// and R2 as packed lower triangles into the rows of par from off_r1 / off_r2, mean(d0) and the packed cov(d0) into init
static int kf_pack_filter(const llpf_model& m, const std::string& at, int f, int F, int nx, int ny, int off_r1, int off_r2,
                          std::vector<double>& par, std::vector<double>& init) {
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
    double S[MAXD * MAXD];
    double* const row[3] = {par.data() + (size_t)off_r1 * F, par.data() + (size_t)off_r2 * F, init.data() + (size_t)nx * F};
    for (int k = 0; k < 3; ++k) {
        gauss_cov_dense(g[k], S);
        for (int r = 0; r < dims[k]; ++r) for (int c = 0; c <= r; ++c) row[k][(size_t)llpf_kf_idx(r, c) * F + f] = S[r * dims[k] + c];
    }
    for (int i = 0; i < nx; ++i) init[(size_t)i * F + f] = m.initial_density.mu[i];
    return LLPF_OK;
}

// the descriptor the model's own methods read (`at`: the filter's message prefix); positive definiteness of R1, R2, cov(d0)
static int kf_model_descriptor(const llpf_model& m, const std::string& at, ModelD* d) {
    const int rc = model_prepare(&m, d);
    if (rc == -1) return fail(LLPF_ERR_ARG, at + "R1 (dynamics_density) is not positive definite");
    if (rc == -2) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
    if (rc == -3) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
    if (rc) return fail(LLPF_ERR_ARG, at + "invalid model descriptor, code " + std::to_string(rc));
    return LLPF_OK;
}

// The pack of a bank whose filters are driven by a model's own functions (the unscented and the extended bank): models -> the descriptors
// ModelD[F], the SoA covariances par [np(nx) + np(ny)][F] (R1 packed, then R2 packed) and the initial state; every check that needs no
// device.  `who`: the prefix of every message; `filter_name`: what the Rao-Blackwellized ids are said not to have; `need_traits`: the
// optional members (LLPF_TRAIT_DYNAMICS_JAC, LLPF_TRAIT_MEASUREMENT_JAC) a compiled model must define for this bank; `allow_traits`: which
// of LLPF_TRAIT_NOISE and LLPF_TRAIT_INITIAL the bank admits (the ensemble bank draws through the model's own members; the others: 0)
static int kf_pack_models(const char* who, const char* filter_name, int need_traits, int allow_traits, const llpf_model* models, int32_t F, int& model_id, int& nx,
                          int& ny, int& nu, std::vector<ModelD>& hm, std::vector<double>& par, std::vector<double>& init) {
    const std::string w = std::string(who) + ": ";
    if (!models) return fail(LLPF_ERR_ARG, w + "models is null");
    if (F < 1) return fail(LLPF_ERR_ARG, w + "n_filters must be >= 1");
    model_id = models[0].model_id; nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (model_id == LLPF_MODEL_RB_LINEAR || model_id == LLPF_MODEL_RB_BILINEAR)
        return fail(LLPF_ERR_ARG, w + "the Rao-Blackwellized models (LLPF_MODEL_RB_LINEAR, LLPF_MODEL_RB_BILINEAR) have no " + filter_name);
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, w + "nx must be in 1..8, ny in 1..4 and nu in 0..8");
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2 || nu != 2) return fail(LLPF_ERR_ARG, w + "the quad-tank has 4 states, 2 outputs and 2 inputs");
    } else if (model_id >= LLPF_MODEL_USER_BASE) {
        std::string src;
        int sx = 0, sy = 0;
        if (!jit_model_source(model_id, src, sx, sy)) return fail(LLPF_ERR_ARG, w + "unknown model id " + std::to_string(model_id));
        if (sx != nx || sy != ny) return fail(LLPF_ERR_ARG, w + "nx, ny differ from the dimensions the model was compiled for");
        const int traits = jit_model_traits(model_id);
        if (traits & LLPF_TRAIT_LOGLIK) return fail(LLPF_ERR_ARG, w + "the model has a likelihood of its own (loglik): there is no Gaussian R2");
        if (traits & LLPF_TRAIT_NOISE & ~allow_traits) return fail(LLPF_ERR_ARG, w + "the model forms its own noise (noise): only additive noise is supported");
        if (traits & LLPF_TRAIT_INITIAL & ~allow_traits) return fail(LLPF_ERR_ARG, w + "the model has an initial density of its own (initial): d0 must be Gaussian");
        if (need_traits & LLPF_TRAIT_DYNAMICS_JAC & ~traits)
            return fail(LLPF_ERR_ARG, w + "the model has no dynamics_jac(x, fx, J): add the member to the snippet, or trace the callable with jacobians = true");
        if (need_traits & LLPF_TRAIT_MEASUREMENT_JAC & ~traits)
            return fail(LLPF_ERR_ARG, w + "the model has no measurement_jac(x, gx, J): add the member to the snippet, or trace the callable with jacobians = true");
    } else if (model_id != LLPF_MODEL_LINEAR_GAUSSIAN) {
        return fail(LLPF_ERR_ARG, w + "unknown model id " + std::to_string(model_id));
    }
    const int np = LLPF_KF_NP(nx), npar = np + LLPF_KF_NP(ny), nstate = nx + np + 1;
    hm.resize((size_t)F);
    par.assign((size_t)npar * F, 0.0);
    init.assign((size_t)nstate * F, 0.0);
    for (int f = 0; f < F; ++f) {
        const llpf_model& m = models[f];
        const std::string at = w + "filter " + std::to_string(f) + ": ";
        if (m.model_id != model_id || m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "model id or dimensions differ from filter 0's");
        CHK(kf_pack_filter(m, at, f, F, nx, ny, 0, np, par, init));
        CHK(kf_model_descriptor(m, at, &hm[(size_t)f]));
    }
    return LLPF_OK;
}

// the device, the dimensions (b.nx, ny, nu are the pack's) and the stream of a new bank; `site`: the bank's create site of test_throw
static int kf_open(KfBank& b, int32_t device, int32_t F, int npar, const char* site) {
    CHK(open_stream(b, device));
    test_throw(site);
    b.F = F;
    b.np = LLPF_KF_NP(b.nx);
    b.npar = npar;
    b.nstate = b.nx + b.np + 1;
    return LLPF_OK;
}

// ---- the banks whose filters are driven by a model's own functions (host/ukf.hpp, host/ekf.hpp) ----
// Next to the bank: the model descriptors ModelD[F] as a bank of particle filters keeps them (the model's own parameters) and a zero
// input; par is [np(nx) + np(ny)][F] (R1, R2 packed, from the llpf_model covariances as given — GaussD keeps a factor, not the covariance)
struct KfModelBank : KfBank {
    const char* filter_name;          // kf_pack_models: what the Rao-Blackwellized ids are said not to have
    int need_traits;                  // ... and the optional members a compiled model must define for this bank
    int allow_traits = 0;             // ... and which of `noise` and `initial` it admits (host/enkf.hpp)
    int model_id = 0;
    double Ts = 1.0;
    DevBuf<ModelD> d_models;
    DevBuf<double> d_zero;
    KfModelBank(const char* who_, const char* filter_name_, int need_traits_) : KfBank(who_), filter_name(filter_name_), need_traits(need_traits_) {}
};

// the descriptors (hm empty: the bank has none) and the constants of a bank to the device, at its creation (`create`) also the zero input
// that goes with the descriptors and the initial state b.h_init; synchronised
static int kf_upload(KfBank& b, DevBuf<ModelD>& d_models, DevBuf<double>& d_zero, const std::vector<ModelD>& hm, const std::vector<double>& par,
                     bool create) {
    HIPC(hipSetDevice(b.device));
    if (create) {
        if (!hm.empty()) {
            CHK(d_models.ensure(hm.size()));
            CHK(d_zero.ensure(MAXU));
            HIPC(hipMemsetAsync(d_zero, 0, sizeof(double) * MAXU, b.stream));
        }
        CHK(b.d_par.ensure(par.size()));
        CHK(b.d_state.ensure(b.h_init.size()));
        HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    }
    if (!hm.empty()) HIPC(hipMemcpyAsync(d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// `site`: the bank's create site of test_throw; prepare(model_id, nx, ny, err): the bank's kernel of a run-time compiled model, on the
// first bank of that model
static int kf_model_create(KfModelBank& b, int32_t device, const llpf_model* models, int32_t F, const char* site,
                           int (*prepare)(int, int, int, std::string&)) {
    std::vector<ModelD> hm;
    std::vector<double> par;
    CHK(kf_pack_models(b.who, b.filter_name, b.need_traits, b.allow_traits, models, F, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_KF_NP(b.nx) + LLPF_KF_NP(b.ny), site));
    b.Ts = models[0].Ts;
    {
        std::string err;
        if (prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, std::string(b.who) + ": " + err);
    }
    return kf_upload(b, b.d_models, b.d_zero, hm, par, true);
}

static int kf_model_set_models(KfModelBank& b, const llpf_model* models) {
    std::vector<ModelD> hm;
    std::vector<double> par, init;
    int id = 0, nx = 0, ny = 0, nu = 0;
    CHK(kf_pack_models(b.who, b.filter_name, b.need_traits, b.allow_traits, models, b.F, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu) return kf_fail(b.who, "set_models must keep the model id and the dimensions of the bank");
    CHK(kf_upload(b, b.d_models, b.d_zero, hm, par, false));
    b.h_init.swap(init);
    b.Ts = models[0].Ts;
    return LLPF_OK;
}

static int kf_reset(KfBank& b) {
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// x [F][nx], R [F][nx][nx] (either may be NULL) of the current state
static int kf_get_state(KfBank& b, double* x, double* R) {
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
static int kf_set_state(KfBank& b, const double* x, const double* R) {
    if (!x || !R) return kf_fail(b.who, "x and R must both be given");
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

// the checks of a run's arguments that need no device (run and smooth of every bank); `out_type`: the name of the outputs' struct
template <class Out>
static int kf_check_run(const KfBank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, const Out* out,
                        const char* out_type = "llpf_kalman_outputs") {
    if (T < 1) return kf_fail(b.who, "T must be >= 1");
    if (!Y) return kf_fail(b.who, "Y is null");
    if (b.nu > 0 && !U) return kf_fail(b.who, "U is null");
    if (per_filter & ~3) return kf_fail(b.who, "per_filter has bits other than 0 and 1");
    if (out && out->struct_size < sizeof(Out)) return kf_fail(b.who, (std::string(out_type) + ".struct_size too small (ABI)").c_str());
    return LLPF_OK;
}

// what a run gives back, as its bank lists it for kf_forward: the outputs of one step in staging order (dst null: not asked for; width:
// doubles per filter) and ll_total [F] (or null), which is row ll_row of the state at every ll_every-th column
struct KfOutputs {
    static constexpr int MAX = 7;
    int n;
    double* dst[MAX];
    uint64_t width[MAX];
    double* ll_total;
    int ll_row, ll_every;
};
// ... of the banks of one filter per column: ll, x, xt, R, Rt, e, and the running sum behind x and the packed R
static KfOutputs kf_outputs(const KfBank& b, double* ll_total, const llpf_kalman_outputs* out) {
    const uint64_t nx = (uint64_t)b.nx;
    const llpf_kalman_outputs none{};
    if (!out) out = &none;
    return {6, {out->ll_steps, out->x, out->xt, out->R, out->Rt, out->e}, {1, nx, nx, nx * nx, nx * nx, (uint64_t)b.ny}, ll_total, b.nx + b.np, 1};
}

// one chunk of the forward pass, as its launcher gets it: steps [t0, t0 + tc) of the run
struct KfChunk {
    const double *u, *y;      // the chunk's inputs on the device (u null: the model has none)
    double* out[KfOutputs::MAX];   // ... and where its outputs are staged, in the run's KfOutputs order, each null when not asked for
    int64_t t0;
    int32_t tc;
    int32_t first;            // 1: the first chunk of the run
    int32_t upf, ypf;         // 1: u / y is per filter
    double* post;             // null, or where the posterior of the chunk's steps goes: [tc][nx + np][F]
};

// the members that the forward argument structs name alike (KalmanArgs, and KfModelArgs through kf_model_args below), from the bank and
// one chunk
template <class Args>
static void kf_fill_args(Args& a, const KfBank& b, const KfChunk& c) {
    a.par = b.d_par; a.state = b.d_state;
    a.u = c.u;
    a.y = c.y;
    double** slot[6] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.e};
    for (int k = 0; k < 6; ++k) *slot[k] = c.out[k];
    a.F = b.F; a.Tc = c.tc; a.nu = b.nu;
    a.u_per = c.upf; a.y_per = c.ypf;
    a.first = c.first;
}

// the arguments of one chunk that the kernels of the model-driven banks have in common
static KfModelArgs kf_model_args(const KfModelBank& b, const KfChunk& c, double t_index0) {
    KfModelArgs a{};
    kf_fill_args(a, b, c);
    a.zero_u = b.d_zero;
    a.t0 = c.t0;
    a.t_index0 = t_index0; a.Ts = b.Ts;
    return a;
}

// the forward pass of a run (arguments checked); post: null, or the device array [T][nx + np][F] that receives the posterior of every
// step.  o: the bank's outputs (kf_outputs; the columns of an IMM bank are lanes, F * o.ll_every of them).  launch(const KfChunk&) fills
// the bank's kernel arguments and launches on b.stream (a status).  Everything is allocated before the first launch.
template <class Launch>
static int kf_forward(KfBank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, const KfOutputs& o, double* post,
                      Launch&& launch) {
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu;
    const bool upf = nu > 0 && (per_filter & 1), ypf = (per_filter & 2) != 0;
    uint64_t w = 0;
    std::vector<ChunkOut> outs;
    for (int k = 0; k < o.n; ++k) {
        if (o.dst[k]) w += o.width[k];
        outs.push_back({o.dst[k], 1, (size_t)F * o.width[k]});
    }
    const uint64_t in_w = (upf ? (uint64_t)nu : 0) + (ypf ? (uint64_t)ny : 0);
    uint64_t total = 0, in_total = 0;      // the per-step outputs / per-filter inputs of all filters and steps, in doubles
    if (!doubles_fit({(uint64_t)F, w, (uint64_t)T}, total) || !doubles_fit({(uint64_t)F, in_w, (uint64_t)T}, in_total))
        return kf_fail(b.who, "the size of the outputs or of the inputs overflows");
    const size_t ncol = (size_t)F * o.ll_every;
    std::vector<double> h_ll(o.ll_total && o.ll_every > 1 ? ncol : 0);      // (the same number in every lane of a filter)
    HIPC(hipSetDevice(b.device));
    ChunkPipe pipe(b.stream);
    // (shared inputs and no per-step outputs: nothing per step scales with F, the chunk is CHUNK_STEPS)
    CHK(pipe.open(T, (size_t)F * (w + in_w) * sizeof(double), outs,
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}, {Y, ypf ? (size_t)F : 0, (size_t)ny, true}}));
    for (int64_t c = 0; c < pipe.nchunk; ++c) {
        CHK(pipe.begin(c, c));
        KfChunk ch{};
        ch.u = pipe.in(0);
        ch.y = pipe.in(1);
        for (int k = 0; k < o.n; ++k) ch.out[k] = pipe.out(k);
        ch.t0 = pipe.t0; ch.tc = (int32_t)pipe.tc;
        ch.first = c == 0 ? 1 : 0;
        ch.upf = upf ? 1 : 0; ch.ypf = ypf ? 1 : 0;
        ch.post = post ? post + (size_t)pipe.t0 * (nx + b.np) * F : nullptr;
        CHK(launch(ch));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    if (o.ll_total)   // the running sum
        HIPC(hipMemcpyAsync(h_ll.empty() ? o.ll_total : h_ll.data(), b.d_state.p + (size_t)o.ll_row * ncol, sizeof(double) * ncol,
                            hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    for (size_t f = 0; f < h_ll.size() / o.ll_every; ++f) o.ll_total[f] = h_ll[f * o.ll_every];
    return LLPF_OK;
}

// one chunk of the backward pass, as its launcher gets it: steps [t0, t0 + tc), run from the last down
struct KfSmoothChunk {
    const double* post;       // [tc][nx + np][F] the posterior of the chunk's steps
    double* carry;            // [nx + np][F] xT, packed RT between the chunks
    const double* u;          // the chunk's inputs on the device (null: the model has none)
    double *xT, *RT;          // where its outputs are staged, each null when not asked for
    int64_t t0;
    int32_t tc;
    int32_t upf;              // 1: u is per filter
    int32_t init;             // 1: the chunk holds the run's last step
};

// the members that KalmanSmoothArgs and UkfSmoothArgs name alike, from the bank and one chunk
template <class Args>
static void kf_fill_smooth_args(Args& a, const KfBank& b, const KfSmoothChunk& c) {
    a.par = b.d_par;
    a.post = c.post;
    a.carry = c.carry;
    a.u = c.u;
    a.xT = c.xT;
    a.RT = c.RT;
    a.F = b.F; a.Tc = c.tc; a.nu = b.nu;
    a.u_per = c.upf;
    a.init = c.init;
}

// smooth(f, u, y) of every filter (the run's arguments checked): the forward pass of a run (the same chunks, outputs and state) that also
// stores the packed posterior of every step on the device (d_post: (nx + np) * 8 bytes per filter-step), then the backward pass over the
// chunks in reverse through a staging pipeline of its own (host/pipe.hpp).  `site`: the bank's smooth site of test_throw; prepare():
// what the bank's kernels need before their first launch (a status); forward(post): the bank's kf_forward; launch(const KfSmoothChunk&):
// as kf_forward's.  Everything is allocated before the first launch, so a call that cannot get its memory leaves the state as it was.
// The state after the call is the one a run leaves (the prior of step T and the running ll).
template <class Prepare, class Forward, class Launch>
static int kf_smooth(KfBank& b, const double* U, int64_t T, int32_t per_filter, const llpf_kalman_smooth_outputs* out, const char* site,
                     Prepare&& prepare, Forward&& forward, Launch&& launch) {
    if (out && out->struct_size < sizeof(llpf_kalman_smooth_outputs))
        return kf_fail(b.who, "llpf_kalman_smooth_outputs.struct_size too small (ABI)");
    const int F = b.F, nx = b.nx, nu = b.nu, ns = nx + b.np;
    const bool upf = nu > 0 && (per_filter & 1);
    double* dst[2] = {out ? out->xT : nullptr, out ? out->RT : nullptr};
    const uint64_t width[2] = {(uint64_t)nx, (uint64_t)nx * nx};
    const uint64_t w = (dst[0] ? width[0] : 0) + (dst[1] ? width[1] : 0);
    uint64_t post_d = 0, total = 0;
    if (!doubles_fit({(uint64_t)ns, (uint64_t)F, (uint64_t)T}, post_d) || !doubles_fit({(uint64_t)F, w, (uint64_t)T}, total))
        return kf_fail(b.who, "the size of the stored posterior or of the smoothed outputs overflows");
    test_throw(site);
    if (!w) return forward(nullptr);     // nothing smoothed is asked for: a run
    HIPC(hipSetDevice(b.device));
    CHK(prepare());
    CHK(b.d_post.ensure((size_t)post_d));
    ChunkPipe pipe(b.stream);
    double* d_carry = nullptr;
    CHK(pipe.device((size_t)ns * F, d_carry));
    CHK(pipe.open(T, (size_t)F * (w + (upf ? nu : 0)) * sizeof(double), {{dst[0], 1, (size_t)F * width[0]}, {dst[1], 1, (size_t)F * width[1]}},
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}}));
    // the forward pass allocates its own staging before its first launch: no launch has run when it returns an allocation failure
    CHK(forward(b.d_post.p));
    for (int64_t i = 0; i < pipe.nchunk; ++i) {      // backward: launch i runs chunk nchunk - 1 - i
        CHK(pipe.begin(i, pipe.nchunk - 1 - i));
        KfSmoothChunk ch{};
        ch.post = b.d_post.p + (size_t)pipe.t0 * ns * F;
        ch.carry = d_carry;
        ch.u = pipe.in(0);
        ch.xT = pipe.out(0);
        ch.RT = pipe.out(1);
        ch.t0 = pipe.t0; ch.tc = (int32_t)pipe.tc;
        ch.upf = upf ? 1 : 0;
        ch.init = i == 0 ? 1 : 0;
        CHK(launch(ch));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
