// kernels/ukf.hpp — k_ukf, k_ukf_smooth: banks of unscented Kalman filters (llpf_ukf_bank_run, llpf_ukf_bank_smooth; host side:
// host/ukf.hpp).  Part of k_ukf.hip (namespace llpf), and the text of the run-time programs of a user model's k_ukf and k_ukf_smooth
// (jit_ukf.inc).
// ------------------------------------------------------------------------------------------------
// One thread per filter, the time loop inside the kernel, x and the packed lower triangle of R in registers — k_kalman's shape.  The step
// is shared/llpf_ukf.h with literal NX, NY (every loop over the dimensions and over the 2 NX + 1 points unrolls) around
// Model::measurement / Model::dynamics, one evaluation per point and stage, so a host build of that header around the same model
// functions gives the same bits.  The model reads its own descriptor ModelD[f] as in k_simulate; R1 and R2 come from the SoA [entry][F].
// Where the mapped points live (UKF_POINTS_LDS): at most 2 NX + 1 points of max(NX, NY) doubles per lane.  Up to NX = 4 — every
// precompiled shape, 36 doubles — they are a local array that unrolling turns into registers; from NX = 5 they are [point][d][lane] in
// LDS, lane fastest (8-byte accesses of a wave cover 64 consecutive doubles: conflict-free), 68 KiB at NX = 8 with the one wave of a
// workgroup.  DESIGN.md 7 has the resource table.
// ------------------------------------------------------------------------------------------------
#ifndef UKF_POINTS_LDS
#define UKF_POINTS_LDS(nx, ny) ((nx) >= 5)
#endif

// POST: also store the posterior of every step for the backward pass (UkfArgs::post; a run without it compiles to the kernel it was — a
// nullable pointer instead costs registers: LinGauss<3, 3> 248 -> 256+16 VGPRs and two waves per SIMD -> one)
template <class Model, int NX, int NY, bool POST = false>
__global__ __launch_bounds__(KF_BLOCK) void k_ukf(const ModelD* __restrict__ models, UkfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no unscented filter");
    constexpr int NP = LLPF_KF_NP(NX), NPT = LLPF_UKF_NPTS(NX), ZD = NX > NY ? NX : NY;
    constexpr bool LDS = UKF_POINTS_LDS(NX, NY);
    __shared__ double zsh[LDS ? NPT * ZD * KF_BLOCK : 1];
    double zreg[LDS ? 1 : NPT * ZD];
    double* Z = LDS ? zsh + threadIdx.x : zreg;
    constexpr int64_t ZS = LDS ? KF_BLOCK : 1;
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const ModelD* md = models + f;
    const double* __restrict__ P = a.par + f;
    double* st = a.state + f;
    double x[NX], R[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) R[i] = st[(NX + i) * F];
    double llt = a.first ? 0.0 : st[(NX + NP) * F];
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
        } else {
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
        if (POST) {                   // SoA: lane f writes column f of each line
            double* q = a.post + (size_t)k * (NX + NP) * F + f;
#pragma unroll
            for (int d = 0; d < NX; ++d) q[d * F] = x[d];
#pragma unroll
            for (int i = 0; i < NP; ++i) q[(NX + i) * F] = R[i];
        }
        {
            const int ok = llpf_ukf_factor(NX, R, Cf);
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                double X[NX], Xn[NX];
                llpf_ukf_point(NX, a.gamma, x, Cf, i, X);
                model.dynamics(X, Xn);
#pragma unroll
                for (int d = 0; d < NX; ++d) Z[(i * NX + d) * ZS] = Xn[d];
            }
            llpf_ukf_predict_finish(NX, a.wm0, a.wc0, a.wi, P, F, ok, Z, ZS, x, R);
        }
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = R[i];
    st[(NX + NP) * F] = llt;
}

// k_ukf_smooth: the backward pass of the unscented RTS smoother (llpf_ukf_bank_smooth), k_kalman_smooth's shape around k_ukf's predict
// stage: one thread per filter, the chunk's steps from last to first inside the kernel.  The smoothed xT and packed RT of the step after
// the chunk come in through `carry` and stay in registers; each step reads the stored posterior (SoA, lane f at column f) and its U row,
// maps the points of the posterior through Model::dynamics — one evaluation per point, into Z as k_ukf keeps it — and is
// llpf_ukf_smooth_finish with literal NX.  The measurement is not used: a model type's NY only rides in the type.  Outputs are
// time-major [Tc][F][...] like k_ukf's.
template <class Model, int NX>
__global__ __launch_bounds__(KF_BLOCK) void k_ukf_smooth(const ModelD* __restrict__ models, UkfSmoothArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no unscented filter");
    constexpr int NP = LLPF_KF_NP(NX), NPT = LLPF_UKF_NPTS(NX);
    constexpr bool LDS = UKF_POINTS_LDS(NX, 0);
    __shared__ double zsh[LDS ? NPT * NX * KF_BLOCK : 1];
    double zreg[LDS ? 1 : NPT * NX];
    double* Z = LDS ? zsh + threadIdx.x : zreg;
    constexpr int64_t ZS = LDS ? KF_BLOCK : 1;
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const ModelD* md = models + f;
    const double* __restrict__ P = a.par + f;
    double* st = a.carry + f;
    double xT[NX], RT[NP];
    const double* last = a.init ? a.post + (size_t)(a.Tc - 1) * (NX + NP) * F + f : st;
#pragma unroll
    for (int d = 0; d < NX; ++d) xT[d] = last[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) RT[i] = last[(NX + i) * F];
    Model model;
#pragma unroll 1
    for (int k = a.Tc - 1; k >= 0; --k) {
        const size_t kf = (size_t)k * F + f;
        if (!(a.init && k == a.Tc - 1)) {
            const double* q = a.post + (size_t)k * (NX + NP) * F + f;
            double xt[NX], Rt[NP], Cf[NP];
#pragma unroll
            for (int d = 0; d < NX; ++d) xt[d] = q[d * F];
#pragma unroll
            for (int i = 0; i < NP; ++i) Rt[i] = q[(NX + i) * F];
            const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.zero_u;
            const double tau = (a.t_index0 + (double)(a.t0 + k)) * a.Ts;
            model.prepare(md, u, tau);
            const int ok = llpf_ukf_factor(NX, Rt, Cf);
#pragma unroll
            for (int i = 0; i < NPT; ++i) {
                double X[NX], Xn[NX];
                llpf_ukf_point(NX, a.gamma, xt, Cf, i, X);
                model.dynamics(X, Xn);
#pragma unroll
                for (int d = 0; d < NX; ++d) Z[(i * NX + d) * ZS] = Xn[d];
            }
            llpf_ukf_smooth_finish(NX, a.gamma, a.wm0, a.wc0, a.wi, P, F, ok, Cf, Z, ZS, xt, Rt, xT, RT);
        }
        if (a.xT) kf_store<NX>(a.xT + kf * NX, xT);
        if (a.RT) kf_store_dense<NX>(a.RT + kf * NX * NX, RT);
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = xT[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = RT[i];
}
