/* llpf_quadtank_jac.h — the quad-tank's discrete-time map (reference examples/example_quadtank.jl:8-35 through rk4 of src/utils.jl:220-237)
 * together with its Jacobian, from ONE evaluation: what QuadTank::dynamics_jac (kernels/models.hpp) and the host shim of the tests run, the
 * same text, so a host build (-ffp-contract=off) is the device's bits.
 *
 * Plain C for host and device.  The value part performs QuadTank::dynamics' operations in dynamics' order (fx is its bits).  No llpf_fma
 * anywhere: the model's own arithmetic is plain IEEE multiplications and additions, and the derivative keeps to that, so that a traced
 * callable's forward-mode Jacobian (tracing.py) is the same kind of expression.  Sums run over their index in increasing order.
 *
 * Structure.  The right-hand side is xd_i = a_i s_i (+ b_i s_{i+2} for i < 2) + inputs, s_i = sqrt(max(tg h_i, 0) + eps), so its derivative D
 * has the six entries (0,0) (0,2) (1,1) (1,3) (2,2) (3,3) with ds_i/dh_i = (tg h_i > 0) ? tg / (2 s_i) : 0.  That pattern (the identity plus the
 * edges 0 <- 2, 1 <- 3) is closed under products, so every stage matrix and the step's Jacobian have it: six numbers each, in the order of
 * LLPF_QT_J*, and no structural zero is ever multiplied out.  One RK4 step:
 *     K1 = D(x),  K2 = D(x + h/2 f1)(I + h/2 K1),  K3 = D(x + h/2 f2)(I + h/2 K2),  K4 = D(x + h f3)(I + h K3),
 *     J_step = I + h/6 (((K1 + 2 K2) + 2 K3) + K4)      (the sum in the order of the state's own update)
 * and the supersamples chain: J = J_step(last) ... J_step(first), the coefficient of s_1 switching after tsw exactly where rhs switches. */
#ifndef LLPF_QUADTANK_JAC_H
#define LLPF_QUADTANK_JAC_H

#include "llpf_detmath.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define LLPF_QT_UNROLL _Pragma("unroll")
#else
#define LLPF_QT_UNROLL
#endif

/* the coefficients of the right-hand side in the reference's evaluation order, (-a/A), (a/A), (gamma k / A), and the step sizes: on the
 * device ModelD::qtc (formed once on the host, host/densities.hpp), on the host llpf_qt_coef_set below — the same expressions */
typedef struct llpf_qt_coef {
    double c1a, c1a_sw, c1b, c1u, c2a, c2b, c2u, c3a, c3u, c4a, c4u;
    double tg, eps, tsw, h, h2, h6;
    int ss;
} llpf_qt_coef;

/* qt: the sixteen constants of llpf_model::qt (LLPF_QT_* order: k1 k2 g A1..A4 a1..a4 gamma1 gamma2 t_switch a1_factor eps) */
LLPF_HD void llpf_qt_coef_set(const double* qt, const double Ts, const int supersample, llpf_qt_coef* c) {
    const double k1 = qt[0], k2 = qt[1], g = qt[2], A1 = qt[3], A2 = qt[4], A3 = qt[5], A4 = qt[6];
    const double a1 = qt[7], a2 = qt[8], a3 = qt[9], a4 = qt[10], g1 = qt[11], g2 = qt[12];
    c->c1a = (-a1) / A1;
    c->c1a_sw = (-(a1 * qt[14])) / A1;
    c->c1b = a3 / A1;
    c->c1u = (g1 * k1) / A1;
    c->c2a = (-a2) / A2;
    c->c2b = a4 / A2;
    c->c2u = (g2 * k2) / A2;
    c->c3a = (-a3) / A3;
    c->c3u = ((1.0 - g2) * k2) / A3;
    c->c4a = (-a4) / A4;
    c->c4u = ((1.0 - g1) * k1) / A4;
    c->tg = 2.0 * g;
    c->eps = qt[15];
    c->tsw = qt[13];
    c->ss = supersample < 1 ? 1 : supersample;
    c->h = Ts / (double)c->ss;
    c->h2 = c->h / 2.0;
    c->h6 = c->h / 6.0;
}

/* the six entries of a matrix of the pattern */
#define LLPF_QT_J00 0
#define LLPF_QT_J02 1
#define LLPF_QT_J11 2
#define LLPF_QT_J13 3
#define LLPF_QT_J22 4
#define LLPF_QT_J33 5
#define LLPF_QT_NNZ 6

/* the right-hand side xd [4] at (h, t) — QuadTank::rhs — and its derivative D [6] */
LLPF_HD void llpf_qt_rhs_jac(const llpf_qt_coef* c, const double u0, const double u1, const double* h, const double t, double* xd, double* D) {
    double s[4], ds[4];
    LLPF_QT_UNROLL
    for (int i = 0; i < 4; ++i) {
        const double v = c->tg * h[i];
        s[i] = llpf_sqrt_pos((v > 0.0 ? v : 0.0) + c->eps);
        ds[i] = v > 0.0 ? c->tg / (2.0 * s[i]) : 0.0;
    }
    const double ca = (t > c->tsw) ? c->c1a_sw : c->c1a;
    xd[0] = ca * s[0] + c->c1b * s[2] + c->c1u * u0;
    xd[1] = c->c2a * s[1] + c->c2b * s[3] + c->c2u * u1;
    xd[2] = c->c3a * s[2] + c->c3u * u1;
    xd[3] = c->c4a * s[3] + c->c4u * u0;
    D[LLPF_QT_J00] = ca * ds[0];
    D[LLPF_QT_J02] = c->c1b * ds[2];
    D[LLPF_QT_J11] = c->c2a * ds[1];
    D[LLPF_QT_J13] = c->c2b * ds[3];
    D[LLPF_QT_J22] = c->c3a * ds[2];
    D[LLPF_QT_J33] = c->c4a * ds[3];
}

/* M = D (I + a K): the stage matrix from the derivative at the stage's point and the previous stage matrix */
LLPF_HD void llpf_qt_stage(const double* D, const double a, const double* K, double* M) {
    const double q00 = 1.0 + a * K[LLPF_QT_J00], q02 = a * K[LLPF_QT_J02], q11 = 1.0 + a * K[LLPF_QT_J11], q13 = a * K[LLPF_QT_J13];
    const double q22 = 1.0 + a * K[LLPF_QT_J22], q33 = 1.0 + a * K[LLPF_QT_J33];
    M[LLPF_QT_J00] = D[LLPF_QT_J00] * q00;
    M[LLPF_QT_J02] = D[LLPF_QT_J00] * q02 + D[LLPF_QT_J02] * q22;
    M[LLPF_QT_J11] = D[LLPF_QT_J11] * q11;
    M[LLPF_QT_J13] = D[LLPF_QT_J11] * q13 + D[LLPF_QT_J13] * q33;
    M[LLPF_QT_J22] = D[LLPF_QT_J22] * q22;
    M[LLPF_QT_J33] = D[LLPF_QT_J33] * q33;
}

/* fx [4] = f(x0) at (u0, u1, t0) and J [r * 4 + c] = d f_r / d x0_c (the ten structural zeros stored as 0.0) */
LLPF_HD void llpf_qt_dynamics_jac(const llpf_qt_coef* c, const double u0, const double u1, const double t0, const double* x0, double* fx,
                                  double* J) {
    double x[4], f1[4], f2[4], f3[4], f4[4], xt[4];
    double K1[LLPF_QT_NNZ], K2[LLPF_QT_NNZ], K3[LLPF_QT_NNZ], K4[LLPF_QT_NNZ], D[LLPF_QT_NNZ], Jt[LLPF_QT_NNZ], Js[LLPF_QT_NNZ];
    double t = t0;
    LLPF_QT_UNROLL
    for (int i = 0; i < 4; ++i) x[i] = x0[i];
    Jt[LLPF_QT_J00] = 1.0; Jt[LLPF_QT_J02] = 0.0; Jt[LLPF_QT_J11] = 1.0; Jt[LLPF_QT_J13] = 0.0; Jt[LLPF_QT_J22] = 1.0; Jt[LLPF_QT_J33] = 1.0;
    for (int it = 0; it < c->ss; ++it) {
        llpf_qt_rhs_jac(c, u0, u1, x, t, f1, K1);
        LLPF_QT_UNROLL
        for (int i = 0; i < 4; ++i) xt[i] = x[i] + c->h2 * f1[i];
        llpf_qt_rhs_jac(c, u0, u1, xt, t + c->h2, f2, D);
        llpf_qt_stage(D, c->h2, K1, K2);
        LLPF_QT_UNROLL
        for (int i = 0; i < 4; ++i) xt[i] = x[i] + c->h2 * f2[i];
        llpf_qt_rhs_jac(c, u0, u1, xt, t + c->h2, f3, D);
        llpf_qt_stage(D, c->h2, K2, K3);
        LLPF_QT_UNROLL
        for (int i = 0; i < 4; ++i) xt[i] = x[i] + c->h * f3[i];
        llpf_qt_rhs_jac(c, u0, u1, xt, t + c->h, f4, D);
        llpf_qt_stage(D, c->h, K3, K4);
        LLPF_QT_UNROLL
        for (int i = 0; i < 4; ++i) x[i] = x[i] + c->h6 * (((f1[i] + 2.0 * f2[i]) + 2.0 * f3[i]) + f4[i]);
        LLPF_QT_UNROLL
        for (int i = 0; i < LLPF_QT_NNZ; ++i) Js[i] = c->h6 * (((K1[i] + 2.0 * K2[i]) + 2.0 * K3[i]) + K4[i]);
        Js[LLPF_QT_J00] = 1.0 + Js[LLPF_QT_J00];
        Js[LLPF_QT_J11] = 1.0 + Js[LLPF_QT_J11];
        Js[LLPF_QT_J22] = 1.0 + Js[LLPF_QT_J22];
        Js[LLPF_QT_J33] = 1.0 + Js[LLPF_QT_J33];
        /* Jt = Js Jt */
        const double n02 = Js[LLPF_QT_J00] * Jt[LLPF_QT_J02] + Js[LLPF_QT_J02] * Jt[LLPF_QT_J22];
        const double n13 = Js[LLPF_QT_J11] * Jt[LLPF_QT_J13] + Js[LLPF_QT_J13] * Jt[LLPF_QT_J33];
        Jt[LLPF_QT_J00] = Js[LLPF_QT_J00] * Jt[LLPF_QT_J00];
        Jt[LLPF_QT_J11] = Js[LLPF_QT_J11] * Jt[LLPF_QT_J11];
        Jt[LLPF_QT_J22] = Js[LLPF_QT_J22] * Jt[LLPF_QT_J22];
        Jt[LLPF_QT_J33] = Js[LLPF_QT_J33] * Jt[LLPF_QT_J33];
        Jt[LLPF_QT_J02] = n02;
        Jt[LLPF_QT_J13] = n13;
        t = t + c->h;
    }
    LLPF_QT_UNROLL
    for (int i = 0; i < 4; ++i) fx[i] = x[i];
    LLPF_QT_UNROLL
    for (int i = 0; i < 16; ++i) J[i] = 0.0;
    J[0] = Jt[LLPF_QT_J00]; J[2] = Jt[LLPF_QT_J02]; J[5] = Jt[LLPF_QT_J11]; J[7] = Jt[LLPF_QT_J13]; J[10] = Jt[LLPF_QT_J22]; J[15] = Jt[LLPF_QT_J33];
}

#endif /* LLPF_QUADTANK_JAC_H */
