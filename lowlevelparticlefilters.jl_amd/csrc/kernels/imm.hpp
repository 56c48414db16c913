// kernels/imm.hpp — the step of a bank of interacting-multiple-model filters, one frame for every kind of mode (imm_chunk), and k_imm: the
// bank over Kalman filters with constant matrices (llpf_imm_bank_run; host side: host/imm.hpp).  Part of k_imm.hip (namespace llpf) and,
// for k_imm_ekf (kernels/imm_ekf.hpp: the bank over extended Kalman filters), of k_imm_ekf.hip and of the text of that kernel's run-time
// programs (jit_imm_ekf.inc).
// ------------------------------------------------------------------------------------------------
// One lane per (filter, mode): G = 1, 2 or 4 lanes per filter, aligned to G, thread f * G + j is mode j of filter f.  The time loop is
// inside the kernel; the lane's x_j, packed R_j and mu_j are in registers, no LDS and no barrier.  The constants are SoA [entry][F * G]:
// a lane's column is its thread index and a wave reads whole lines.  The step is the six stages of shared/llpf_imm.h; stages 2 and 6, the
// mode's own correct! and predict!, are the Mode's (below: ImmKalmanMode; kernels/imm_ekf.hpp: ImmEkfMode), everything else is here.
//
// The exchange.  What the step of shared/llpf_imm.h sums over the source mode i — mu_i, a_i, w_i, x_i, R_i — a lane fetches from lane i of
// its group, i = 0 .. M - 1 in that order, and does the header's arithmetic on it: a lane's bits are those of the host loop.  A group lies
// inside one quad, so the fetch is a quad permute (DPP through the compiler's builtin, a double as two halves): the compiler keeps the DPP
// hazards.
//
// Fetch uniformity (the invariant of this file).  Every imm_fetch sits in control flow that is uniform over the group, with all G lanes
// of the group active: the branches around a fetch test only the launch's M, interact and outputs and the filter's missing row, never a
// lane's own numbers.  A mode's own branches (a lost definiteness, a model's switch time, a snippet's `if` or loop) are per lane; they
// live inside the Mode's begin / correct / predict, which are called between the fetches and have reconverged when they return.  No
// fetch may move into a block conditioned on per-lane data (cj == 0, a NaN ll, `on`), nor into a Mode.
//
// Idle lanes (M = 3 in G = 4).  Lane 3 of a group runs along on finite numbers, is never a source (every loop over the source mode stops
// at M) and stores nothing.  Its column of P is zero, so its c_j is 0 and it is never mixed.  Which column it runs on is the Mode's
// (IDLE_ON_MODE0): its own, which the host leaves zero, or mode 0's where a zero column is not safe to compute on.
// ------------------------------------------------------------------------------------------------
#ifndef KF_RELOAD
#define KF_RELOAD(nx, ny) ((nx) >= 5)
#endif

// v of lane I of the group (G == 2: the quad is two groups)
template <int G, int I>
DEV double imm_lane(double v) {
    constexpr int ctrl = G == 4 ? I * 0x55 : (I | (I << 2) | ((2 + I) << 4) | ((2 + I) << 6));
    const uint64_t u = llpf_d2u(v);
    const int lo = (int)(uint32_t)u, hi = (int)(uint32_t)(u >> 32);
    const int l2 = __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xF, 0xF, false);
    const int h2 = __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xF, 0xF, false);
    return llpf_u2d(((uint64_t)(uint32_t)h2 << 32) | (uint64_t)(uint32_t)l2);
}
// v of lane i < G of the group (i is a literal once the loops over the modes are unrolled)
template <int G>
DEV double imm_fetch(double v, int i) {
    if constexpr (G == 1) return v;
    else if constexpr (G == 2) return i == 0 ? imm_lane<2, 0>(v) : imm_lane<2, 1>(v);
    else return i == 0 ? imm_lane<4, 0>(v) : i == 1 ? imm_lane<4, 1>(v) : i == 2 ? imm_lane<4, 2>(v) : imm_lane<4, 3>(v);
}

// xm = sum_i w[i] x_i, Rm = sum_i w[i] (R_i + (x_i - xm)(x_i - xm)') over the modes of the group (llpf_imm_mean_add, llpf_imm_cov_add with
// mode i's state fetched entry by entry)
template <int NX, int G>
DEV void imm_weighted(const int M, const double* w, const double* x, const double* R, double* xm, double* Rm) {
    constexpr int NP = LLPF_KF_NP(NX);
#pragma unroll
    for (int d = 0; d < NX; ++d) xm[d] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) Rm[i] = 0.0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i < M) {
#pragma unroll
            for (int r = 0; r < NX; ++r) xm[r] = llpf_imm_mean_term(w[i], imm_fetch<G>(x[r], i), xm[r]);
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (i < M) {
            double d[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) d[r] = imm_fetch<G>(x[r], i) - xm[r];
#pragma unroll
            for (int r = 0; r < NX; ++r) {
#pragma unroll
                for (int c = 0; c <= r; ++c)
                    Rm[llpf_kf_idx(r, c)] = llpf_imm_cov_term(w[i], imm_fetch<G>(R[llpf_kf_idx(r, c)], i), d[r], d[c], Rm[llpf_kf_idx(r, c)]);
            }
        }
    }
}

// mu_i of every mode of the group into mu_all, and c_j = sum_i P_ij mu_i of this lane's mode
template <int G>
DEV double imm_c(const int M, const double* Pc, double mu, double* mu_all) {
    double c = 0.0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        mu_all[i] = 0.0;
        if (i < M) {
            mu_all[i] = imm_fetch<G>(mu, i);
            c = llpf_imm_c_add(Pc[i], mu_all[i], c);
        }
    }
    return c;
}

// A chunk of steps of this thread's lane.  Mode: the kind of filter a mode is, constructed by the kernel from its own arguments —
//   IDLE_ON_MODE0        an idle lane reads mode 0's column and a zero column of P (false: its own, zero, column)
//   npar(nu)             the rows of par in front of column j of P
//   no_u()               what stands in for u when the model has no inputs
//   begin(P, col, u, k)  once per step, before stage 1: the constants of step k (P: the lane's column of par)
//   missing(y)           the filter's row is missing (uniform over the group)
//   correct(Pk, L, u, y, missing, x, R) -> ll_j   and   predict(Pk, L, u, x, R): stages 2 and 6 on the lane's own x_j, R_j
// (a: by value.  Through a reference to the kernel's own argument the compiler leaves the tests of the launch's outputs inside the time
// loop: k_imm measured 2 to 3.5 % slower at F = 10^4.)
template <int NX, int NY, int G, class Mode>
DEV void imm_chunk(const ImmBaseArgs a, Mode& mode) {
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F, L = F * G;
    const int64_t t = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (t >= L) return;                   // whole groups: KF_BLOCK is a multiple of G
    const int64_t f = t / G;
    const int j = (int)(t % G);
    const int nu = a.nu, M = a.M;
    const bool on = j < M;
    const bool own = on || !Mode::IDLE_ON_MODE0;
    const int64_t col = own ? t : t - j;
    const double* __restrict__ P = a.par + col;
    double* st = a.state + col;
    double Pc[G];
#pragma unroll
    for (int i = 0; i < G; ++i) Pc[i] = own ? P[(int64_t)(mode.npar(nu) + i) * L] : 0.0;
    double x[NX], R[NP];
#pragma unroll
    for (int d = 0; d < NX; ++d) x[d] = st[d * L];
#pragma unroll
    for (int i = 0; i < NP; ++i) R[i] = st[(NX + i) * L];
    double mu = st[(NX + NP) * L];
    double llt = a.first ? 0.0 : st[(NX + NP + 1) * L];
#pragma unroll 1
    for (int k = 0; k < a.Tc; ++k) {
        const size_t kf = (size_t)k * F + f;
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : mode.no_u();
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
        const double* Pk = mode.begin(P, col, u, k);
        double mu_all[G], xc[NX], Rc[NP];
        // 1. the combined prior
        if (a.x || a.R) {
#pragma unroll
            for (int i = 0; i < G; ++i) mu_all[i] = i < M ? imm_fetch<G>(mu, i) : 0.0;
            imm_weighted<NX, G>(M, mu_all, x, R, xc, Rc);
            if (j == 0 && a.x) kf_store<NX>(a.x + kf * NX, xc);
            if (j == 0 && a.R) kf_store_dense<NX>(a.R + kf * NX * NX, Rc);
        }
        // 2. correct! of the lane's mode
        const bool missing = mode.missing(y);
        const double llj = mode.correct(Pk, L, u, y, missing, x, R);
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
        // 6. predict! of the lane's mode
        mode.predict(Pk, L, u, x, R);
    }
    if (!on) return;
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * L] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * L] = R[i];
    st[(NX + NP) * L] = mu;
    st[(NX + NP + 1) * L] = llt;
}

// A Kalman filter with constant matrices: shared/llpf_kalman.h with literal NX, NY on the lane's own parameter column, exactly as k_kalman
// runs it (correct! sees a missing row itself: ll_j = 0).  An idle lane runs along on its own zero column.
template <int NX, int NY>
struct ImmKalmanMode {
    static constexpr bool IDLE_ON_MODE0 = false;
    const ImmArgs& a;
    DEV int npar(int nu) const { return LLPF_KF_NPAR(NX, NY, nu); }
    DEV const double* no_u() const { return a.u; }
    DEV const double* begin(const double* P, int64_t, const double*, int k) const { return KF_RELOAD(NX, NY) ? P + (size_t)k * a.par_tstride : P; }
    DEV bool missing(const double* y) const { return !(y[0] == y[0]); }
    DEV double correct(const double* Pk, int64_t L, const double* u, const double* y, bool, double* x, double* R) const {
        double e[NY];
        return llpf_kf_correct(NX, NY, a.nu, Pk, L, u, y, x, R, e);
    }
    DEV void predict(const double* Pk, int64_t L, const double* u, double* x, double* R) const { llpf_kf_predict(NX, NY, a.nu, Pk, L, u, x, R); }
};

template <int NX, int NY, int G>
__global__ __launch_bounds__(KF_BLOCK) void k_imm(ImmArgs a) {
    ImmKalmanMode<NX, NY> mode{a};
    imm_chunk<NX, NY, G>(a, mode);
}
