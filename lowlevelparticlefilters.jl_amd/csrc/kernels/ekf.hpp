// kernels/ekf.hpp — k_ekf: banks of extended and of iterated extended Kalman filters (llpf_ekf_bank_run; host side: host/ekf.hpp).  Part
// of k_ekf.hip (namespace llpf), and the text of the run-time programs of a user model's two kernels (jit_ekf.inc).
// ------------------------------------------------------------------------------------------------
// One thread per filter, the time loop inside the kernel, x and the packed lower triangle of R in registers — k_kalman's and k_ukf's
// shape.  The step is shared/llpf_ekf.h with literal NX, NY (every loop over the dimensions unrolls) around Model::measurement_jac /
// Model::dynamics_jac, ONE evaluation of the model and its Jacobian per stage, so a host build of that header around the same model
// functions gives the same bits.  The model reads its own descriptor ModelD[f] as in k_simulate; R1 and R2 come from the SoA [entry][F].
// There are no sigma points, so nothing lives in LDS: value, Jacobian (NX * NX doubles at most) and the step's temporaries are local
// arrays that unrolling turns into registers.  DESIGN.md 7 has the resource table.
// The argument type picks the filter.  k_ekf<Model, NX, NY> (EkfArgs) is the plain one.  k_ekf<Model, NX, NY, IekfArgs> is the iterated
// one: the iterated correct! of llpf_ekf.h (llpf_iekf_iterate until llpf_iekf_stop) in the place of llpf_ekf_correct.  The prior stays
// in x, R while the iterate and its covariance live in registers of their own, and the iteration is a loop that is not unrolled, one
// measurement_jac per pass.  The lanes of a wave stop after different numbers of passes: the wave runs until its slowest lane stops, the
// others masked off.
// ------------------------------------------------------------------------------------------------
template <class Model, int NX, int NY, class Args = EkfArgs>
__global__ __launch_bounds__(KF_BLOCK) void k_ekf(const ModelD* __restrict__ models, Args a) {
    constexpr bool ITERATED = Args::ITERATED;
    static_assert(!Model::RB, "the Rao-Blackwellized models have no extended Kalman filter");
    static_assert(has_dynamics_jac<Model>::value, "an extended Kalman filter needs Model::dynamics_jac(x, fx, J)");
    static_assert(has_measurement_jac<Model>::value, "an extended Kalman filter needs Model::measurement_jac(x, gx, J)");
    constexpr int NP = LLPF_KF_NP(NX);
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
        double e[NY], ll = 0.0;
        if (llpf_ekf_missing(y)) {            // a missing row: correct! is skipped
#pragma unroll
            for (int r = 0; r < NY; ++r) e[r] = llpf_kf_nan();
        } else {
            double gx[NY], C[NY * NX], yr[NY];
            if constexpr (ITERATED) {
                double xi[NX], Rn[NP], move;
#pragma unroll
                for (int r = 0; r < NY; ++r) yr[r] = y[r];
#pragma unroll
                for (int d = 0; d < NX; ++d) xi[d] = x[d];
                int done = 0;
#pragma unroll 1
                do {
                    model.measurement_jac(xi, gx, C);
                    ll = llpf_iekf_iterate(NX, NY, P, F, yr, gx, C, NX, x, R, done == 0, xi, Rn, e, &move);
                    ++done;
                } while (!llpf_iekf_stop(done, a.maxiters, move, a.epsilon));
#pragma unroll
                for (int d = 0; d < NX; ++d) x[d] = xi[d];
#pragma unroll
                for (int i = 0; i < NP; ++i) R[i] = Rn[i];
            } else {
                model.measurement_jac(x, gx, C);
#pragma unroll
                for (int r = 0; r < NY; ++r) yr[r] = y[r];
                ll = llpf_ekf_correct(NX, NY, P, F, yr, gx, C, NX, x, R, e);
            }
        }
        llt = llt + ll;
        if (a.ll) a.ll[kf] = ll;
        if (a.e) kf_store<NY>(a.e + kf * NY, e);
        if (a.xt) kf_store<NX>(a.xt + kf * NX, x);
        if (a.Rt) kf_store_dense<NX>(a.Rt + kf * NX * NX, R);
        {
            double fx[NX], A[NX * NX];
            model.dynamics_jac(x, fx, A);
            llpf_ekf_predict(NX, P, F, fx, A, NX, x, R);
        }
    }
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * F] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * F] = R[i];
    st[(NX + NP) * F] = llt;
}
