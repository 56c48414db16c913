// kernels/sqkf.hpp — k_sqkf: banks of square-root Kalman filters with constant matrices (llpf_sqkf_bank_run; host side: host/sqkf.hpp).
// Part of k_sqkf.hip (namespace llpf).
// ------------------------------------------------------------------------------------------------
// k_kalman's shape (kernels/kalman.hpp): one thread per filter, the time loop inside the kernel, x and the packed factor Lr in registers,
// the constants from the SoA [entry][F] each step, shared or per-filter U / Y rows, time-major outputs.  The step is shared/llpf_sqkf.h
// with literal NX, NY, so a host build of that header gives the same bits.  The arguments are KalmanArgs (post and par_tstride's reload
// trick unused: the constants are read where a pre-array is formed, once per step each).  The pre-arrays of the two triangularisations
// live in registers for every shape: fully unrolled, every entry has a register of its own while it is live (DESIGN.md §7 has the
// register counts per shape).  The R and Rt outputs are llpf_sq_cov of the factor, formed only where they are asked for.
// ------------------------------------------------------------------------------------------------
// (KF_BLOCK, kf_store, kf_store_dense: kernels/kf_store.hpp)
template <int NX, int NY>
__global__ __launch_bounds__(KF_BLOCK) void k_sqkf(KalmanArgs a) {
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const double* __restrict__ P = a.par + f;
    double* st = a.state + f;
    double x[NX], Lr[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) Lr[i] = st[(NX + i) * F];
    double llt = a.first ? 0.0 : st[(NX + NP) * F];
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        if (a.x) kf_store<NX>(a.x + kf * NX, x);
        if (a.R) {
            double R[NP];
            llpf_sq_cov(NX, Lr, R);
            kf_store_dense<NX>(a.R + kf * NX * NX, R);
        }
        double e[NY];
        const double ll = llpf_sq_correct(NX, NY, nu, P, F, u, y, x, Lr, e);
        llt = llt + ll;
        if (a.ll) a.ll[kf] = ll;
        if (a.e) kf_store<NY>(a.e + kf * NY, e);
        if (a.xt) kf_store<NX>(a.xt + kf * NX, x);
        if (a.Rt) {
            double R[NP];
            llpf_sq_cov(NX, Lr, R);
            kf_store_dense<NX>(a.Rt + kf * NX * NX, R);
        }
        llpf_sq_predict(NX, NY, nu, P, F, u, x, Lr);
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = Lr[i];
    st[(NX + NP) * F] = llt;
}
