// kernels/simulate.hpp — k_simulate: M trajectories of the model of every filter (the reference's simulate(pf, T, du), src/filtering.jl:457-477).
// Part of k_simulate.hip (namespace llpf), and the text of the run-time program of a user model's k_simulate (jit_simulate.inc).
// ------------------------------------------------------------------------------------------------
// One thread per trajectory m, the time loop inside the kernel, x in registers:
//   x_0     = mean(d0), or with LLPF_SIM_SAMPLE_INITIAL the draw reset! gives particle m (k_init / k_init_user: LLPF_STREAM_INIT and
//             LLPF_STREAM_USER_INIT at counter (m, step0))
//   y_t     = g(x_t, u_t, p, tau_t) + e_t,  e_t = mu + L xi of measurement_density, xi from LLPF_STREAM_MEASURE at (m, step0 + t)
//             (a model with a likelihood of its own still draws from the Gaussian descriptor: a likelihood has no sampler)
//   x_{t+1} = f(x_t, u_t, p, tau_t) + w_t,  w_t the process noise predict! gives particle m at Philox step step0 + t (k_step: the Gaussian
//             descriptor from LLPF_STREAM_DYNAMICS, or UserModel::noise with the uniforms of LLPF_STREAM_USER)
// Same model methods, same generator, same operation order as k_init / k_step: the same bits by construction.
// Outputs are time-major, [F][Tc][M][nx | ny]: the nx (ny) doubles of a lane are consecutive, so a wave's stores cover whole lines.
// ------------------------------------------------------------------------------------------------
typedef double llpf_sim_d2 __attribute__((ext_vector_type(2)));
template <int ND>
DEV void sim_store(double* p, const double* v, bool nt) {
    if constexpr (ND % 2 == 0) {            // 16-byte stores: p is 16-byte aligned (ND even, the buffer 256-byte aligned)
#pragma unroll
        for (int d = 0; d < ND; d += 2) {
            llpf_sim_d2 w;
            w.x = v[d];
            w.y = v[d + 1];
            if (nt) __builtin_nontemporal_store(w, reinterpret_cast<llpf_sim_d2*>(p + d));
            else *reinterpret_cast<llpf_sim_d2*>(p + d) = w;
        }
    } else {
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            if (nt) __builtin_nontemporal_store(v[d], p + d);
            else p[d] = v[d];
        }
    }
}

template <class Model, int NX, int NY>
__global__ __launch_bounds__(BLOCK) void k_simulate(const ModelD* __restrict__ models, SimArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models are not simulated");
    // the generator's tables in LDS, as k_step keeps them
    __shared__ __attribute__((aligned(16))) double sh_rng_lg[2 * LLPF_RNG_LG_ENTRIES], sh_rng_sc[2 * LLPF_RNG_SC_ENTRIES];
    {
        const int t = (int)threadIdx.x;
        if (t < LLPF_RNG_SC_ENTRIES) { sh_rng_sc[2 * t] = LLPF_SIN64[t]; sh_rng_sc[2 * t + 1] = LLPF_COS64[t]; }
        else if (t < LLPF_RNG_SC_ENTRIES + LLPF_RNG_LG_ENTRIES) {
            sh_rng_lg[2 * (t - LLPF_RNG_SC_ENTRIES)] = LLPF_LOG_INVC[t - LLPF_RNG_SC_ENTRIES];
            sh_rng_lg[2 * (t - LLPF_RNG_SC_ENTRIES) + 1] = LLPF_LOG_LNC[t - LLPF_RNG_SC_ENTRIES];
        }
        __syncthreads();
    }
    const int f = blockIdx.y;
    const int64_t M = a.M;
    const int64_t m = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (m >= M) return;
    const ModelD* md = models + f;
    const uint64_t key = a.key0 + (uint64_t)f * a.key_stride;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const uint32_t idx = (uint32_t)m;
    double* xs = a.xs + (size_t)f * NX * M;
    double x[NX];
    Model model;
    if (a.t0 == 0) {
        if (a.flags & LLPF_SIM_SAMPLE_INITIAL) {
            double xi[NX];
            llpf_normals(idx, a.step0, LLPF_STREAM_INIT, k0, k1, NX, xi);
            if constexpr (has_user_initial<Model>::value) {          // k_init_user
                double uu[NX];
                llpf_uniforms(idx, a.step0, LLPF_STREAM_USER_INIT, k0, k1, NX, uu);
                model.prepare(md, a.zero_u, 0.0);
                model.initial(xi, uu, x);
            } else {
                gauss_sample<NX>(md->d0, xi, x);                      // k_init
            }
        } else {
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = md->d0.mu[d];
        }
    } else {
#pragma unroll
        for (int d = 0; d < NX; ++d) x[d] = xs[(size_t)d * M + m];
    }
    const double* ub = a.nu > 0 ? a.u + (size_t)f * a.u_fstride + (size_t)m * a.u_mstride : a.zero_u;
    const bool nt = a.nt != 0;
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const int64_t t = a.t0 + k;
        const uint32_t step = a.step0 + (uint32_t)t;
        const double tau = (a.t_index0 + (double)t) * a.Ts;
        model.prepare(md, a.nu > 0 ? ub + (size_t)k * a.nu : ub, tau);
        if (a.X) sim_store<NX>(a.X + (((size_t)f * a.Tc + k) * M + m) * NX, x, nt);
        if (a.Y) {
            double y[NY];
            model.measurement(x, y);
            if (a.flags & LLPF_SIM_MEASUREMENT_NOISE) {
                double xi[NY], e[NY];
                llpf_normals_tab(idx, step, LLPF_STREAM_MEASURE, k0, k1, NY, xi, sh_rng_lg, sh_rng_sc);
                gauss_sample<NY>(md->dg, xi, e);
#pragma unroll
                for (int r = 0; r < NY; ++r) y[r] = y[r] + e[r];
            }
            sim_store<NY>(a.Y + (((size_t)f * a.Tc + k) * M + m) * NY, y, nt);
        }
        if (t + 1 >= a.T) break;
        double fx[NX];
        model.dynamics(x, fx);
        if (!(a.flags & LLPF_SIM_DYNAMICS_NOISE)) {
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = fx[d];
        } else if constexpr (has_user_noise<Model>::value) {        // k_step: the model adds its own noise
            double xi[NX], uu[NX];
            llpf_normals_tab(idx, step, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, sh_rng_lg, sh_rng_sc);
            llpf_uniforms(idx, step, LLPF_STREAM_USER, k0, k1, NX, uu);
            double xn[NX];
            model.noise(x, fx, xi, uu, xn);
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = xn[d];
        } else {
            double xi[NX], nz[NX];
            llpf_normals_tab(idx, step, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, sh_rng_lg, sh_rng_sc);
            gauss_sample<NX>(md->df, xi, nz);
#pragma unroll
            for (int d = 0; d < NX; ++d) x[d] = fx[d] + nz[d];
        }
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) xs[(size_t)d * M + m] = x[d];
}
