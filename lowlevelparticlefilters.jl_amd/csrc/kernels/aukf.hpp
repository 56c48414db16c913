// kernels/aukf.hpp — k_aukf: banks of unscented Kalman filters with augmented (non-additive) process noise (llpf_aukf_bank_run; host
// side: host/aukf.hpp).  Part of k_aukf.hip (namespace llpf), and the text of the run-time program of a user model's k_aukf
// (jit_aukf.inc).
// ------------------------------------------------------------------------------------------------
// k_ukf's shape: one thread per filter, the time loop inside the kernel, x, the packed lower triangle of R and the packed factor C1 of
// R1 (formed once, before the loop) in registers.  The step is shared/llpf_aukf.h with literal NX, NY around Model::measurement and
// Model::dynamics_w — or, for a model without that member, Model::dynamics at the 2 NX + 1 distinct state points, the 2 NX noise points
// taking the centre's value plus their noise (the same numbers, so the same bits as evaluating f again) — so a host build of that header
// around the same model functions gives the same bits.
// Where the mapped points live (AUKF_POINTS_LDS): max((2 NX + 1) NY, (4 NX + 1) NX) doubles per lane.  Up to NX = 5 (105 doubles) they
// are a local array that unrolling turns into registers — every precompiled shape, and (5, 1) and (5, 4) compiled for gfx950, use no
// scratch; from NX = 6 (150 doubles), where the local array no longer fits the 512 registers of a lane, they are [point][d][lane] in
// LDS, lane fastest (8-byte accesses of a wave cover 64 consecutive doubles: conflict-free), 132 KiB at NX = 8 with the one wave of a
// workgroup.  DESIGN.md 7 has the resource table.
// ------------------------------------------------------------------------------------------------
#ifndef AUKF_POINTS_LDS
#define AUKF_POINTS_LDS(nx, ny) ((nx) >= 6)
#endif

template <class Model, int NX, int NY>
__global__ __launch_bounds__(KF_BLOCK) void k_aukf(const ModelD* __restrict__ models, AukfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no unscented filter");
    constexpr int NP = LLPF_KF_NP(NX), NPT = LLPF_UKF_NPTS(NX), NPA = LLPF_AUKF_NPTS(NX);
    constexpr int ZN = NPT * NY > NPA * NX ? NPT * NY : NPA * NX;
    constexpr bool LDS = AUKF_POINTS_LDS(NX, NY);
    __shared__ double zsh[LDS ? ZN * KF_BLOCK : 1];
    double zreg[LDS ? 1 : ZN];
    double* Z = LDS ? zsh + threadIdx.x : zreg;
    constexpr int64_t ZS = LDS ? KF_BLOCK : 1;
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const ModelD* md = models + f;
    const double* __restrict__ P = a.par + f;
    double* st = a.state + f;
    double x[NX], R[NP], C1[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) R[i] = st[(NX + i) * F];
    double llt = a.first ? 0.0 : st[(NX + NP) * F];
    const int ok1 = llpf_aukf_noise_factor(NX, P, F, C1);
    Model model;
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.zero_u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        const double tau = (a.t_index0 + (double)(a.t0 + k)) * a.Ts;
        model.prepare(md, u, tau);
        if (a.x) kf_store<NX>(a.x + kf * NX, x);
        if (a.R) kf_store_dense<NX>(a.R + kf * NX * NX, R);
        double e[NY], Cf[NP], ll = 0.0;
        if (!(y[0] == y[0])) {            // a missing row: correct! is skipped
#pragma unroll
            for (int r = 0; r < NY; ++r) e[r] = llpf_kf_nan();
        } else {                          // k_ukf's correct!, call for call, with the measurement set
            const int ok = llpf_ukf_factor(NX, R, Cf);
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                double X[NX], Y[NY];
                llpf_ukf_point(NX, a.gamma, x, Cf, i, X);
                model.measurement(X, Y);
#pragma unroll
                for (int r = 0; r < NY; ++r) Z[(i * NY + r) * ZS] = Y[r];
            }
            double yr[NY];
#pragma unroll
            for (int r = 0; r < NY; ++r) yr[r] = y[r];
            ll = llpf_ukf_correct_finish(NX, NY, a.gamma, a.wm0, a.wc0, a.wi, P, F, ok, Cf, Z, ZS, yr, x, R, e);
        }
        llt = llt + ll;
        if (a.ll) a.ll[kf] = ll;
        if (a.e) kf_store<NY>(a.e + kf * NY, e);
        if (a.xt) kf_store<NX>(a.xt + kf * NX, x);
        if (a.Rt) kf_store_dense<NX>(a.Rt + kf * NX * NX, R);
        {
            const int ok = llpf_ukf_factor(NX, R, Cf) & ok1;
            double f0[NX];                // f at the centre: what the noise points of an additive model reuse
#pragma unroll
            for (int i = 0; i < NPA; ++i) {
                double X[NX], W[NX], Xn[NX];
                const int noise = llpf_aukf_point(NX, a.gamma_a, x, Cf, C1, i, X, W);
                if constexpr (has_dynamics_w<Model>::value) {
                    model.dynamics_w(X, W, Xn);
                } else if (noise) {
                    llpf_aukf_additive(NX, f0, W, Xn);
                } else {
                    model.dynamics(X, Xn);
                    if (i == 0) {
#pragma unroll
                        for (int d = 0; d < NX; ++d) f0[d] = Xn[d];
                    }
                }
#pragma unroll
                for (int d = 0; d < NX; ++d) Z[(i * NX + d) * ZS] = Xn[d];
            }
            llpf_aukf_predict_finish(NX, a.wm0a, a.wc0a, a.wia, ok, Z, ZS, x, R);
        }
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = R[i];
    st[(NX + NP) * F] = llt;
}
