// kernels/enkf.hpp — k_enkf: banks of ensemble Kalman filters (llpf_enkf_bank_*; host side: host/enkf.hpp; step: shared/llpf_enkf.h).
// Part of k_enkf.hip (namespace llpf), and the text of the run-time program of a user model's kernels (jit_enkf.inc).
// ------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per ensemble, the time loop inside the kernel.  Thread tid owns the members i = tid, tid + 256, ... in
// every pass over the ensemble: it is the only one that ever reads or writes them, so the passes of a step need no barrier between a
// store and the next load, and the members live in the device buffer [F][nx][N] (SoA: a wave's loads cover whole lines) between passes
// and between launches.  A step is
//   pass 1   load x_i, Y_i = g(x_i); sum x and Y                                   -> xbar, ybar
//   pass 2   dX_i, dY_i (g evaluated again: the same bits, no scratch plane); sum dX dY', dY dY'   -> L, W, e, ll (llpf_enkf_gain)
//   pass 3   g again, perturb, update (llpf_enkf_member_update), then dynamics and process noise as k_simulate forms them, store
// — three passes when only ll is asked for.  An output that is asked for adds its own passes and reductions (x: none; R: one; xt: the
// update is stored and summed before the dynamics, one more pass; Rt: one more), a missing row without outputs runs pass 3's second
// half alone, inflation adds the sum of the propagated members and a pass that moves them.  No output feeds back.
// A sum over the ensemble is llpf_enkf_sum's tree (shared/llpf_enkf.h): a thread's members added in increasing i into its slot, the 64
// slots of a wave by a butterfly of DPP moves (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: every lane of a row of 16 then holds
// that row's balanced tree; row_bcast 15 and 31 add the rows as (r0 + r1) + (r2 + r3) into lane 63), the four waves through LDS as
// (w0 + w1) + (w2 + w3), which every thread reads back: the broadcast.  Every thread then forms L, W and ll from the same sums (uniform
// arithmetic; nothing is stored between the reduction and its use) and thread 0 stores the step's outputs, time-major as k_ekf's.
// Nothing crosses a workgroup: no atomics, no spin, no grid-wide wait.  The generator's tables sit in LDS as in k_simulate.
// ------------------------------------------------------------------------------------------------
constexpr int ENKF_BLOCK = BLOCK;
static_assert(ENKF_BLOCK == LLPF_ENKF_SLOTS && ENKF_BLOCK == 256, "a thread is a slot of llpf_enkf_sum; four waves");
#define DPP_ROW_MIRROR 0x140

template <int CTRL, int RM>
DEV double enkf_dpp_add(double v) {      // lanes outside the row mask add 0.0
    return v + llpf_u2d(dpp_u64<CTRL, RM, false>(0, llpf_d2u(v)));
}
// the balanced tree over the wave's 64 slots: valid in lane 63
DEV double enkf_wave_sum(double v) {
    v = enkf_dpp_add<DPP_QUAD_XOR1, 0xF>(v);
    v = enkf_dpp_add<DPP_QUAD_XOR2, 0xF>(v);
    v = enkf_dpp_add<DPP_ROW_HALF_MIRROR, 0xF>(v);
    v = enkf_dpp_add<DPP_ROW_MIRROR, 0xF>(v);
    v = enkf_dpp_add<DPP_ROW_BCAST15, 0xA>(v);
    v = enkf_dpp_add<DPP_ROW_BCAST31, 0xC>(v);
    return v;
}
// v[0 .. K): every thread's slots in, the totals out in every thread; sh: 4 K doubles of LDS.  Every thread of the workgroup calls it
template <int K>
DEV void enkf_block_sum(double* v, double* sh) {
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    __syncthreads();                     // the readers of the last call are done with sh
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double t = enkf_wave_sum(v[k]);
        if (lane == 63) sh[k * 4 + wv] = t;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (sh[k * 4] + sh[k * 4 + 1]) + (sh[k * 4 + 2] + sh[k * 4 + 3]);
}

template <int NX>
DEV void enkf_load(const double* xm, int N, int i, double* x) {
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = xm[(size_t)d * N + i];
}
template <int NX>
DEV void enkf_store(double* xm, int N, int i, const double* x) {
#pragma unroll
    for (int d = 0; d < NX; ++d) xm[(size_t)d * N + i] = x[d];
}
// the mean of the ensemble in every thread
template <int NX>
DEV void enkf_mean_pass(const double* xm, int N, double* sh, double* xbar) {
#pragma unroll
    for (int d = 0; d < NX; ++d) xbar[d] = 0.0;
#pragma unroll 1
    for (int i = (int)threadIdx.x; i < N; i += ENKF_BLOCK) {
        double x[NX];
        enkf_load<NX>(xm, N, i, x);
#pragma unroll
        for (int d = 0; d < NX; ++d) xbar[d] = xbar[d] + x[d];
    }
    enkf_block_sum<NX>(xbar, sh);
#pragma unroll
    for (int d = 0; d < NX; ++d) xbar[d] = llpf_enkf_mean(xbar[d], N);
}
// the packed sample covariance about xbar in every thread
template <int NX>
DEV void enkf_cov_pass(const double* xm, int N, double* sh, const double* xbar, double* Rp) {
    constexpr int NP = LLPF_KF_NP(NX);
#pragma unroll
    for (int j = 0; j < NP; ++j) Rp[j] = 0.0;
#pragma unroll 1
    for (int i = (int)threadIdx.x; i < N; i += ENKF_BLOCK) {
        double x[NX];
        enkf_load<NX>(xm, N, i, x);
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = x[d] - xbar[d];
#pragma unroll
        for (int r = 0; r < NX; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c) Rp[llpf_kf_idx(r, c)] = Rp[llpf_kf_idx(r, c)] + x[r] * x[c];
    }
    enkf_block_sum<NP>(Rp, sh);
#pragma unroll
    for (int j = 0; j < NP; ++j) Rp[j] = llpf_enkf_cov(Rp[j], N);
}

// predict! of one member: x = f(x) + w as k_simulate forms it (idx: the member, step: the Philox step)
template <class Model, int NX>
DEV void enkf_propagate(const Model& model, const ModelD* md, uint32_t idx, uint32_t step, uint32_t k0, uint32_t k1, const double* sh_rng_lg,
                        const double* sh_rng_sc, double* x) {
    double fx[NX], xi[NX];
    model.dynamics(x, fx);
    llpf_normals_tab(idx, step, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, sh_rng_lg, sh_rng_sc);
    if constexpr (has_user_noise<Model>::value) {
        double uu[NX], xn[NX];
        llpf_uniforms(idx, step, LLPF_STREAM_USER, k0, k1, NX, uu);
        model.noise(x, fx, xi, uu, xn);
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = xn[d];
    } else {
        double nz[NX];
        gauss_sample<NX>(md->df, xi, nz);
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = fx[d] + nz[d];
    }
}

template <class Model, int NX, int NY>
__global__ __launch_bounds__(ENKF_BLOCK) void k_enkf(const ModelD* __restrict__ models, EnkfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no ensemble Kalman filter");
    constexpr int NP = LLPF_KF_NP(NX), NPY = LLPF_KF_NP(NY);
    constexpr int NRED = NX * NY + NPY > NP ? NX * NY + NPY : NP;      // the most values one reduction carries
    __shared__ __attribute__((aligned(16))) double sh_rng_lg[2 * LLPF_RNG_LG_ENTRIES], sh_rng_sc[2 * LLPF_RNG_SC_ENTRIES];
    __shared__ double sh[4 * NRED];
    const int tid = (int)threadIdx.x;
    {
        if (tid < LLPF_RNG_SC_ENTRIES) { sh_rng_sc[2 * tid] = LLPF_SIN64[tid]; sh_rng_sc[2 * tid + 1] = LLPF_COS64[tid]; }
        else if (tid < LLPF_RNG_SC_ENTRIES + LLPF_RNG_LG_ENTRIES) {
            sh_rng_lg[2 * (tid - LLPF_RNG_SC_ENTRIES)] = LLPF_LOG_INVC[tid - LLPF_RNG_SC_ENTRIES];
            sh_rng_lg[2 * (tid - LLPF_RNG_SC_ENTRIES) + 1] = LLPF_LOG_LNC[tid - LLPF_RNG_SC_ENTRIES];
        }
        __syncthreads();
    }
    const int64_t F = a.F;
    const int64_t f = blockIdx.x;
    const int N = a.N, nu = a.nu;
    const ModelD* md = models + f;
    const double* __restrict__ P = a.par + f;
    double* st = a.state + f;
    double* xm = a.members + (size_t)f * NX * N;
    const uint64_t key = a.key0 + (uint64_t)f;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const bool do_correct = (a.phases & LLPF_ENKF_CORRECT) != 0, do_predict = (a.phases & LLPF_ENKF_PREDICT) != 0;
    const bool inflate = do_predict && a.rho != 1.0;
    const bool want_post = a.xt != nullptr || a.Rt != nullptr;
    double llt = a.first ? 0.0 : st[(NX + NP) * F];
    Model model;
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.zero_u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        const double tau = (a.t_index0 + (double)(a.t0 + k)) * a.Ts;
        const uint32_t step = a.step0 + (uint32_t)(a.t0 + k);
        model.prepare(md, u, tau);
        const bool missing = !do_correct || !(y[0] == y[0]);
        double e[NY], ll = 0.0;
        double L[NPY], inv[NY], W[NY * LLPF_KF_MAXX], yr[NY];
        int ok = 1;
        if (missing) {
#pragma unroll
            for (int r = 0; r < NY; ++r) e[r] = llpf_kf_nan();
            if (a.x || a.R) {                 // the prior's moments are asked for
                double xbar[NX], Rp[NP];
                enkf_mean_pass<NX>(xm, N, sh, xbar);
                if (a.x && tid == 0) kf_store<NX>(a.x + kf * NX, xbar);
                if (a.R) {
                    enkf_cov_pass<NX>(xm, N, sh, xbar, Rp);
                    if (tid == 0) kf_store_dense<NX>(a.R + kf * NX * NX, Rp);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < NY; ++r) yr[r] = y[r];
            // pass 1: the means
            double m[NX + NY];
#pragma unroll
            for (int j = 0; j < NX + NY; ++j) m[j] = 0.0;
#pragma unroll 1
            for (int i = tid; i < N; i += ENKF_BLOCK) {
                double x[NX], Y[NY];
                enkf_load<NX>(xm, N, i, x);
                model.measurement(x, Y);
#pragma unroll
                for (int d = 0; d < NX; ++d) m[d] = m[d] + x[d];
#pragma unroll
                for (int r = 0; r < NY; ++r) m[NX + r] = m[NX + r] + Y[r];
            }
            enkf_block_sum<NX + NY>(m, sh);
#pragma unroll
            for (int j = 0; j < NX + NY; ++j) m[j] = llpf_enkf_mean(m[j], N);
            if (a.x && tid == 0) kf_store<NX>(a.x + kf * NX, m);
            if (a.R) {
                double Rp[NP];
                enkf_cov_pass<NX>(xm, N, sh, m, Rp);
                if (tid == 0) kf_store_dense<NX>(a.R + kf * NX * NX, Rp);
            }
            // pass 2: the centred second moments, sxy [NY][NX] then syy packed
            double s2[NX * NY + NPY];
#pragma unroll
            for (int j = 0; j < NX * NY + NPY; ++j) s2[j] = 0.0;
#pragma unroll 1
            for (int i = tid; i < N; i += ENKF_BLOCK) {
                double x[NX], Y[NY];
                enkf_load<NX>(xm, N, i, x);
                model.measurement(x, Y);
#pragma unroll
                for (int d = 0; d < NX; ++d) x[d] = x[d] - m[d];
#pragma unroll
                for (int r = 0; r < NY; ++r) Y[r] = Y[r] - m[NX + r];
#pragma unroll
                for (int r = 0; r < NY; ++r)
#pragma unroll
                    for (int d = 0; d < NX; ++d) s2[r * NX + d] = s2[r * NX + d] + x[d] * Y[r];
#pragma unroll
                for (int r = 0; r < NY; ++r)
#pragma unroll
                    for (int c = 0; c <= r; ++c) s2[NX * NY + llpf_kf_idx(r, c)] = s2[NX * NY + llpf_kf_idx(r, c)] + Y[r] * Y[c];
            }
            enkf_block_sum<NX * NY + NPY>(s2, sh);
            {
                double sxy[NY * LLPF_KF_MAXX];
#pragma unroll
                for (int r = 0; r < NY; ++r)
#pragma unroll
                    for (int d = 0; d < NX; ++d) sxy[r * LLPF_KF_MAXX + d] = s2[r * NX + d];
                ll = llpf_enkf_gain(NX, NY, N, P, F, sxy, s2 + NX * NY, yr, m + NX, L, inv, W, e, &ok);
            }
        }
        llt = llt + ll;
        if (tid == 0) {
            if (a.ll) a.ll[kf] = ll;
            if (a.e) kf_store<NY>(a.e + kf * NY, e);
        }
        // pass 3: the update and, unless the posterior's moments come between, the dynamics
        const bool fused = !want_post;
        double sx[NX];      // inflation: the sum of the propagated members
#pragma unroll
        for (int d = 0; d < NX; ++d) sx[d] = 0.0;
        if (!missing || (fused && do_predict)) {
#pragma unroll 1
            for (int i = tid; i < N; i += ENKF_BLOCK) {
                double x[NX];
                enkf_load<NX>(xm, N, i, x);
                if (!missing) {
                    double Y[NY], xi[NY], v[NY];
                    model.measurement(x, Y);
                    llpf_normals_tab((uint32_t)i, step, LLPF_STREAM_MEASURE, k0, k1, NY, xi, sh_rng_lg, sh_rng_sc);
                    gauss_sample<NY>(md->dg, xi, v);
                    llpf_enkf_member_update(NX, NY, ok, L, inv, W, yr, Y, v, x);
                }
                if (fused && do_predict) {
                    enkf_propagate<Model, NX>(model, md, (uint32_t)i, step, k0, k1, sh_rng_lg, sh_rng_sc, x);
#pragma unroll
                    for (int d = 0; d < NX; ++d) sx[d] = sx[d] + x[d];
                }
                enkf_store<NX>(xm, N, i, x);
            }
        }
        if (want_post) {
            double xbar[NX], Rp[NP];
            enkf_mean_pass<NX>(xm, N, sh, xbar);
            if (a.xt && tid == 0) kf_store<NX>(a.xt + kf * NX, xbar);
            if (a.Rt) {
                enkf_cov_pass<NX>(xm, N, sh, xbar, Rp);
                if (tid == 0) kf_store_dense<NX>(a.Rt + kf * NX * NX, Rp);
            }
            if (do_predict) {
#pragma unroll 1
                for (int i = tid; i < N; i += ENKF_BLOCK) {
                    double x[NX];
                    enkf_load<NX>(xm, N, i, x);
                    enkf_propagate<Model, NX>(model, md, (uint32_t)i, step, k0, k1, sh_rng_lg, sh_rng_sc, x);
#pragma unroll
                    for (int d = 0; d < NX; ++d) sx[d] = sx[d] + x[d];
                    enkf_store<NX>(xm, N, i, x);
                }
            }
        }
        if (inflate) {
            enkf_block_sum<NX>(sx, sh);
#pragma unroll
            for (int d = 0; d < NX; ++d) sx[d] = llpf_enkf_mean(sx[d], N);
#pragma unroll 1
            for (int i = tid; i < N; i += ENKF_BLOCK) {
                double x[NX];
                enkf_load<NX>(xm, N, i, x);
                llpf_enkf_inflate(NX, a.rho, sx, x);
                enkf_store<NX>(xm, N, i, x);
            }
        }
    }
    // the state the chunk leaves: mean, packed sample covariance, running ll
    {
        double xbar[NX], Rp[NP];
        enkf_mean_pass<NX>(xm, N, sh, xbar);
        enkf_cov_pass<NX>(xm, N, sh, xbar, Rp);
        if (tid == 0) {
#pragma unroll
            for (int d = 0; d < NX; ++d) st[d * F] = xbar[d];
#pragma unroll
            for (int j = 0; j < NP; ++j) st[(NX + j) * F] = Rp[j];
            st[(NX + NP) * F] = llt;
        }
    }
}

// reset! of every ensemble: member i of filter f is the draw k_init / k_init_user gives particle i (grid: ceil(N / 256) x F)
template <class Model, int NX>
__global__ __launch_bounds__(ENKF_BLOCK) void k_enkf_init(const ModelD* __restrict__ models, EnkfInitArgs a) {
    const int f = blockIdx.y;
    const int i = (int)(blockIdx.x * ENKF_BLOCK + threadIdx.x);
    if (i >= a.N) return;
    const ModelD* md = models + f;
    const uint64_t key = a.key0 + (uint64_t)f;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    double xi[NX], x[NX];
    llpf_normals((uint32_t)i, a.n_reset, LLPF_STREAM_INIT, k0, k1, NX, xi);
    if constexpr (has_user_initial<Model>::value) {
        double uu[NX];
        Model model;
        llpf_uniforms((uint32_t)i, a.n_reset, LLPF_STREAM_USER_INIT, k0, k1, NX, uu);
        model.prepare(md, a.zero_u, 0.0);
        model.initial(xi, uu, x);
    } else {
        gauss_sample<NX>(md->d0, xi, x);
    }
    enkf_store<NX>(a.members + (size_t)f * NX * a.N, a.N, i, x);
}

// mean and packed sample covariance of every ensemble into the state [nx + np + 1][F] (after reset! and set_members; zero_ll: the running
// ll restarts); model-free, one workgroup per filter
template <int NX>
__global__ __launch_bounds__(ENKF_BLOCK) void k_enkf_moments(const double* __restrict__ members, double* state, int64_t F, int N, int zero_ll) {
    constexpr int NP = LLPF_KF_NP(NX);
    __shared__ double sh[4 * NP];
    const int64_t f = blockIdx.x;
    const double* xm = members + (size_t)f * NX * N;
    double* st = state + f;
    double xbar[NX], Rp[NP];
    enkf_mean_pass<NX>(xm, N, sh, xbar);
    enkf_cov_pass<NX>(xm, N, sh, xbar, Rp);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d < NX; ++d) st[d * F] = xbar[d];
#pragma unroll
        for (int j = 0; j < NP; ++j) st[(NX + j) * F] = Rp[j];
        if (zero_ll) st[(NX + NP) * F] = 0.0;
    }
}
