// kernels/imm_ekf.hpp — k_imm_ekf: banks of interacting-multiple-model filters whose modes are first-order extended Kalman filters of one
// model type (llpf_imm_bank_run_at on a bank with LLPF_IMM_EXTENDED; host side: host/imm.hpp).  Part of k_imm_ekf.hip (namespace llpf,
// after kernels/imm.hpp), and the text of the run-time program of a user model's kernel (jit_imm_ekf.inc).
// ------------------------------------------------------------------------------------------------
// k_imm's shape: one lane per (filter, mode), G = 1, 2 or 4 lanes per filter, thread f * G + j is mode j of filter f, the time loop inside
// the kernel, the lane's x_j, packed R_j and mu_j in registers, no LDS and no barrier.  The step is the six stages of shared/llpf_imm.h in
// k_imm's order; the mode's own step is shared/llpf_ekf.h with literal NX, NY around Model::measurement_jac (stage 2, at the mode's prior)
// and Model::dynamics_jac (stage 6, at the mode's x after the mixing), as k_ekf runs it: value, Jacobian and the temporaries are local
// arrays.  The model reads the lane's own descriptor ModelD[f * G + j]; R1, R2 and column j of P come from the SoA [entry][F * G].  The
// exchange between the modes is kernels/imm.hpp's imm_fetch / imm_weighted / imm_c: a lane's bits are those of the host loop over the
// two shared headers.
//
// Fetch uniformity (the invariant of this file).  Every imm_fetch sits in control flow that is uniform over the group, with all G lanes
// of the group active: the branches around a fetch test only the launch's M, interact and outputs and the filter's missing row, never a
// lane's own numbers.  A model's own branches (the quad-tank's switch time, a snippet's `if` or loop) are per lane; they live inside
// prepare / measurement_jac / dynamics_jac, which are called between the fetches and have reconverged when they return.  No fetch may
// move into a block conditioned on per-lane data (cj == 0, a NaN ll, `on`).
//
// Idle lanes (M = 3 in G = 4).  Lane 3 of a group runs along on finite numbers: it reads mode 0's column — descriptor, R1, R2 and state —
// so that the model never sees a zero descriptor (a zero divisor, a zero supersample).  Its column of P is zero, so its c_j is 0 and it
// is never mixed; it is never a source (every loop over the source mode stops at M) and it stores nothing.
// ------------------------------------------------------------------------------------------------
template <class Model, int NX, int NY, int G>
__global__ __launch_bounds__(KF_BLOCK) void k_imm_ekf(const ModelD* __restrict__ models, ImmEkfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no extended Kalman filter");
    static_assert(has_dynamics_jac<Model>::value, "an extended Kalman filter needs Model::dynamics_jac(x, fx, J)");
    static_assert(has_measurement_jac<Model>::value, "an extended Kalman filter needs Model::measurement_jac(x, gx, J)");
    constexpr int NP = LLPF_KF_NP(NX);
    constexpr int NPAR = LLPF_EKF_NPAR(NX, NY);
    const int64_t F = a.F, L = F * G;
    const int64_t t = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (t >= L) return;                   // whole groups: KF_BLOCK is a multiple of G
    const int64_t f = t / G;
    const int j = (int)(t % G);
    const int nu = a.nu, M = a.M;
    const bool on = j < M;
    const int64_t col = on ? t : t - j;   // an idle lane reads mode 0's column
    const ModelD* md = models + col;
    const double* __restrict__ P = a.par + col;
    double* st = a.state + col;
    double Pc[G];
#pragma unroll
    for (int i = 0; i < G; ++i) Pc[i] = on ? P[(int64_t)(NPAR + i) * L] : 0.0;
    double x[NX], R[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * L];
#pragma unroll
    for (int i = 0; i < NP; ++i) R[i] = st[(NX + i) * L];
    double mu = st[(NX + NP) * L];
    double llt = a.first ? 0.0 : st[(NX + NP + 1) * L];
    Model model;
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.zero_u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        const double tau = (a.t_index0 + (double)(a.t0 + k)) * a.Ts;
        model.prepare(md, u, tau);
        double mu_all[G], xc[NX], Rc[NP];
        // 1. the combined prior
        if (a.x || a.R) {
#pragma unroll
            for (int i = 0; i < G; ++i) mu_all[i] = i < M ? imm_fetch<G>(mu, i) : 0.0;
            imm_weighted<NX, G>(M, mu_all, x, R, xc, Rc);
            if (j == 0 && a.x) kf_store<NX>(a.x + kf * NX, xc);
            if (j == 0 && a.R) kf_store_dense<NX>(a.R + kf * NX * NX, Rc);
        }
        // 2. correct! of the lane's mode: one measurement_jac at the prior x_j (a missing row: skipped, ll_j = 0)
        const bool missing = llpf_ekf_missing(y);      // the filter's: uniform over the group
        double llj = 0.0;
        if (!missing) {
            double gx[NY], C[NY * NX], yr[NY], e[NY];
            model.measurement_jac(x, gx, C);
#pragma unroll
            for (int r = 0; r < NY; ++r) yr[r] = y[r];
            llj = llpf_ekf_correct(NX, NY, P, L, yr, gx, C, NX, x, R, e);
        }
        // 3. the mode probabilities
        const double c = imm_c<G>(M, Pc, mu, mu_all);
        double ll = 0.0;
        if (missing) {
            mu = c;
        } else {
            const double aj = llpf_imm_loga(c, llj);
            double m = imm_fetch<G>(aj, 0);
#pragma unroll
            for (int i = 1; i < G; ++i) {
                if (i < M) m = llpf_imm_max(m, imm_fetch<G>(aj, i));
            }
            const double w = llpf_imm_w(c, aj, m);
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                if (i < M) s = s + imm_fetch<G>(w, i);
            }
            ll = llpf_imm_ll(m, s);
            mu = w / s;
            llpf_imm_poison(NX, ll, x, R);
        }
        llt = llt + ll;
        if (j == 0 && a.ll) a.ll[kf] = ll;
        if (on && a.mu) a.mu[kf * M + j] = mu;
        if (on && a.ll_modes) a.ll_modes[kf * M + j] = llj;
        // 4. the combined posterior
        if (a.xt || a.Rt) {
#pragma unroll
            for (int i = 0; i < G; ++i) mu_all[i] = i < M ? imm_fetch<G>(mu, i) : 0.0;
            imm_weighted<NX, G>(M, mu_all, x, R, xc, Rc);
            if (j == 0 && a.xt) kf_store<NX>(a.xt + kf * NX, xc);
            if (j == 0 && a.Rt) kf_store_dense<NX>(a.Rt + kf * NX * NX, Rc);
        }
        // 5. the mixing: this lane's mode from the modes as they are
        if (a.interact) {
            const double cj = imm_c<G>(M, Pc, mu, mu_all);
            double wm[G];
#pragma unroll
            for (int i = 0; i < G; ++i) wm[i] = llpf_imm_mix_w(Pc[i], mu_all[i], cj);
            imm_weighted<NX, G>(M, wm, x, R, xc, Rc);
            if (!(cj == 0.0)) {           // (a mode without mass is not mixed)
#pragma unroll
                for (int d = 0; d < NX; ++d) x[d] = xc[d];
#pragma unroll
                for (int i = 0; i < NP; ++i) R[i] = Rc[i];
            }
        }
        // 6. predict! of the lane's mode: one dynamics_jac at x_j after the mixing
        {
            double fx[NX], A[NX * NX];
            model.dynamics_jac(x, fx, A);
            llpf_ekf_predict(NX, P, L, fx, A, NX, x, R);
        }
    }
    if (!on) return;
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * L] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * L] = R[i];
    st[(NX + NP) * L] = mu;
    st[(NX + NP + 1) * L] = llt;
}
