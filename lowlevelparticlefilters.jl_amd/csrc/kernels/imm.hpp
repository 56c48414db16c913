// kernels/imm.hpp — k_imm: banks of interacting-multiple-model filters over Kalman filters with constant matrices (llpf_imm_bank_run; host
// side: host/imm.hpp).  Part of k_imm.hip (namespace llpf); its exchange (imm_fetch, imm_weighted, imm_c) is also k_imm_ekf's: the file is
// part of k_imm_ekf.hip and of the text of that kernel's run-time programs (jit_imm_ekf.inc) as well.
// ------------------------------------------------------------------------------------------------
// One lane per (filter, mode): G = 1, 2 or 4 lanes per filter, aligned to G, thread f * G + j is mode j of filter f (M = 3 runs in G = 4
// with one idle lane, which stores nothing and is never a source).  The time loop is inside the kernel; the lane's x_j and packed R_j are
// in registers and its correct! / predict! are shared/llpf_kalman.h with literal NX, NY on the lane's own parameter column, exactly as
// k_kalman runs them.  The constants are SoA [entry][F * G]: a lane's column is its thread index and a wave reads whole lines.
//
// The exchange.  What the step of shared/llpf_imm.h sums over the source mode i — mu_i, a_i, w_i, x_i, R_i — a lane fetches from lane i of
// its group, i = 0 .. M - 1 in that order, and does the header's arithmetic on it: a lane's bits are those of the host loop.  A group lies
// inside one quad, so the fetch is a quad permute (DPP through the compiler's builtin, a double as two halves): no LDS, no barrier, and
// the compiler keeps the DPP hazards.  Every branch that holds a fetch is uniform over the group (M, interact and the outputs asked for
// are the launch's, a missing row is the filter's); the branches on a lost definiteness are per lane and hold none.
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

template <int NX, int NY, int G>
__global__ __launch_bounds__(KF_BLOCK) void k_imm(ImmArgs a) {
    constexpr int NP = LLPF_KF_NP(NX);
    const int64_t F = a.F, L = F * G;
    const int64_t t = (int64_t)blockIdx.x * KF_BLOCK + threadIdx.x;
    if (t >= L) return;                   // whole groups: KF_BLOCK is a multiple of G
    const int64_t f = t / G;
    const int j = (int)(t % G);
    const int nu = a.nu, M = a.M;
    const bool on = j < M;                // (an idle lane runs along on its zero column)
    const double* __restrict__ P0 = a.par + t;
    double* st = a.state + t;
    double Pc[G];
#pragma unroll
    for (int i = 0; i < G; ++i) Pc[i] = P0[(int64_t)(LLPF_KF_NPAR(NX, NY, nu) + i) * L];
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
        const double* u = nu > 0 ? a.u + (a.u_per ? kf : (size_t)k) * nu : a.u;
        const double* y = a.y + (a.y_per ? kf : (size_t)k) * NY;
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
        double e[NY];
        const double* P = KF_RELOAD(NX, NY) ? P0 + (size_t)k * a.par_tstride : P0;
        const double llj = llpf_kf_correct(NX, NY, nu, P, L, u, y, x, R, e);
        // 3. the mode probabilities
        const double c = imm_c<G>(M, Pc, mu, mu_all);
        double ll = 0.0;
        if (!(y[0] == y[0])) {
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
        llpf_kf_predict(NX, NY, nu, P, L, u, x, R);
    }
    if (!on) return;
#pragma unroll
    for (int d = 0; d < NX; ++d) st[d * L] = x[d];
#pragma unroll
    for (int i = 0; i < NP; ++i) st[(NX + i) * L] = R[i];
    st[(NX + NP) * L] = mu;
    st[(NX + NP + 1) * L] = llt;
}
