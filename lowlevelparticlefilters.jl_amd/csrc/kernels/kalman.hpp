// kernels/kalman.hpp — k_kalman: banks of Kalman filters with constant matrices (llpf_kalman_bank_run; host side: host/kalman.hpp).
// Part of k_kalman.hip (namespace llpf).
// ------------------------------------------------------------------------------------------------
// One thread per filter, the time loop inside the kernel, x and the packed lower triangle of R in registers.  The step is
// shared/llpf_kalman.h with literal NX, NY (every loop over the dimensions unrolls; nu is a run-time number), so a host build of that
// header gives the same bits.  The constant matrices are read from the SoA [entry][F] each step (lane f at column f: a wave reads whole
// lines); shared U / Y rows are one address for every lane, per-filter rows come time-major [Tc][F][n].  Outputs are time-major
// [Tc][F][...], a lane's n doubles consecutive.
// ------------------------------------------------------------------------------------------------
// (KF_BLOCK, kf_store, kf_store_dense: kernels/kf_store.hpp, shared with k_ukf)
#ifndef KF_RELOAD
#define KF_RELOAD(nx, ny) ((nx) >= 5)
#endif

// POST: also store the posterior of every step for the backward pass (KalmanArgs::post; a run without it compiles to the kernel it was)
template <int NX, int NY, bool POST>
__global__ __launch_bounds__(KF_BLOCK) void k_kalman(KalmanArgs a) {
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const double* __restrict__ P0 = a.par + f;
    double* st = a.state + f;
    double x[NX], R[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) R[i] = st[(NX + i) * F];
    double llt = a.first ? 0.0 : st[(NX + NP) * F];
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        if (a.x) kf_store<NX>(a.x + kf * NX, x);
        if (a.R) kf_store_dense<NX>(a.R + kf * NX * NX, R);
        double e[NY];
        // (KF_RELOAD: par_tstride is a run-time 0, so the constants' addresses look step-dependent and their loads stay inside the loop)
        const double* P = KF_RELOAD(NX, NY) ? P0 + (size_t)k * a.par_tstride : P0;
        const double ll = llpf_kf_correct(NX, NY, nu, P, F, u, y, x, R, e);
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
        llpf_kf_predict(NX, NY, nu, P, F, u, x, R);
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = R[i];
    st[(NX + NP) * F] = llt;
}

// k_kalman_smooth: the backward pass of the RTS smoother (llpf_kalman_bank_smooth), one thread per filter, the chunk's steps from last to
// first inside the kernel.  The smoothed xT and packed RT of the step after the chunk come in through `carry` and stay in registers; each
// step reads the stored posterior (SoA, like the constants) and its U row and is llpf_kf_smooth with literal NX (ny and nu at run time:
// ny only moves the offsets of R1 and B).  Outputs are time-major [Tc][F][...] like k_kalman's.
template <int NX>
__global__ __launch_bounds__(KF_BLOCK) void k_kalman_smooth(KalmanSmoothArgs a) {
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int ny = a.ny, nu = a.nu;
    const double* __restrict__ P0 = a.par + f;
    double* st = a.carry + f;
    double xT[NX], RT[NP];
    const double* last = a.init ? a.post + (size_t)(a.Tc - 1) * (NX + NP) * F + f : st;
#pragma unroll
    for (int d = 0; d < NX; ++d) xT[d] = last[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) RT[i] = last[(NX + i) * F];
#pragma unroll 1
    for (int k = a.Tc - 1; k >= 0; --k) {
        const size_t kf = (size_t)k * F + f;
        if (!(a.init && k == a.Tc - 1)) {
            const double* q = a.post + (size_t)k * (NX + NP) * F + f;
            double xt[NX], Rt[NP];
#pragma unroll
            for (int d = 0; d < NX; ++d) xt[d] = q[d * F];
#pragma unroll
            for (int i = 0; i < NP; ++i) Rt[i] = q[(NX + i) * F];
            const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.u;
            const double* P = KF_RELOAD(NX, 0) ? P0 + (size_t)k * a.par_tstride : P0;
            llpf_kf_smooth(NX, ny, nu, P, F, u, xt, Rt, xT, RT);
        }
        if (a.xT) kf_store<NX>(a.xT + kf * NX, xT);
        if (a.RT) kf_store_dense<NX>(a.RT + kf * NX * NX, RT);
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = xT[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = RT[i];
}
