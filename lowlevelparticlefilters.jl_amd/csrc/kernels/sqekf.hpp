// kernels/sqekf.hpp — k_sqekf: banks of square-root extended Kalman filters (llpf_sqekf_bank_run; host side: host/sqekf.hpp).  Part of
// k_sqekf.hip (namespace llpf), and the text of the run-time program of a user model's kernel (jit_sqekf.inc).
// ------------------------------------------------------------------------------------------------
// k_ekf's frame (kernels/ekf.hpp): one thread per filter, the time loop inside the kernel, ONE evaluation of the model and its Jacobian
// per stage (Model::measurement_jac / Model::dynamics_jac), shared or per-filter U / Y rows, tau = (t_index0 + t0 + k) Ts, time-major
// outputs.  The step is shared/llpf_sqekf.h with literal NX, NY, so a host build of that header around the same model functions gives the
// same bits.  As in k_sqkf (kernels/sqkf.hpp) the state rows nx .. nx + np - 1 hold the packed factor Lr of R, the pre-arrays of the two
// triangularisations are local arrays whose dimensions are literals (unrolled, every entry has a register of its own while it is live;
// the largest shapes spill, DESIGN.md 7 has the resource table), and the R and Rt outputs are llpf_sq_cov of the factor, formed only
// where they are asked for.  The arguments are KfModelArgs as they stand: the filter has none of its own.
// ------------------------------------------------------------------------------------------------
template <class Model, int NX, int NY>
__global__ __launch_bounds__(KF_BLOCK) void k_sqekf(const ModelD* __restrict__ models, KfModelArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no square-root extended Kalman filter");
    static_assert(has_dynamics_jac<Model>::value, "a square-root extended Kalman filter needs Model::dynamics_jac(x, fx, J)");
    static_assert(has_measurement_jac<Model>::value, "a square-root extended Kalman filter needs Model::measurement_jac(x, gx, J)");
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F;
    const int64_t f = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int nu = a.nu;
    const ModelD* md = models + f;
    const double* __restrict__ P = a.par + f;
    double* st = a.state + f;
    double x[NX], Lr[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * F];
#pragma unroll
    for (int i = 0; i < NP; ++i) Lr[i] = st[(NX + i) * F];
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
        if (a.R) {
            double R[NP];
            llpf_sq_cov(NX, Lr, R);
            kf_store_dense<NX>(a.R + kf * NX * NX, R);
        }
        double e[NY], ll = 0.0;
        if (llpf_ekf_missing(y)) {            // a missing row: correct! is skipped
#pragma unroll
            for (int r = 0; r < NY; ++r) e[r] = llpf_kf_nan();
        } else {
            double gx[NY], C[NY * NX], yr[NY];
            model.measurement_jac(x, gx, C);
#pragma unroll
            for (int r = 0; r < NY; ++r) yr[r] = y[r];
            ll = llpf_sqekf_correct(NX, NY, P, F, yr, gx, C, NX, x, Lr, e);
        }
        llt = llt + ll;
        if (a.ll) a.ll[kf] = ll;
        if (a.e) kf_store<NY>(a.e + kf * NY, e);
        if (a.xt) kf_store<NX>(a.xt + kf * NX, x);
        if (a.Rt) {
            double R[NP];
            llpf_sq_cov(NX, Lr, R);
            kf_store_dense<NX>(a.Rt + kf * NX * NX, R);
        }
        {
            double fx[NX], A[NX * NX];
            model.dynamics_jac(x, fx, A);
            llpf_sqekf_predict(NX, P, F, fx, A, NX, x, Lr);
        }
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = Lr[i];
    st[(NX + NP) * F] = llt;
}
