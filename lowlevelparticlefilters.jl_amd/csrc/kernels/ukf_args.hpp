// kernels/ukf_args.hpp — arguments of k_ukf and k_ukf_smooth (kernels/ukf.hpp).  Included inside namespace llpf by engine.hpp (host side)
// and compiled into the run-time programs of a model's k_ukf and k_ukf_smooth (k_ukf.hip, jit_ukf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F unscented Kalman filters, one thread per filter.  Device arrays are SoA /
// time-major as k_kalman's: a wave's 64 lanes read and write whole lines.
struct UkfArgs {
    const double* par;       // [np(nx) + np(ny)][F] R1, R2 as packed lower triangles (shared/llpf_ukf.h: LLPF_UKF_OFF_*)
    double* state;           // [nx + np + 1][F] x, packed R, the run's running ll_total: in at t0, out at t0 + Tc
    const double* u;         // inputs of the chunk: [Tc][nu] shared, or [Tc][F][nu] (u_per = 1); unused when nu = 0
    const double* y;         // measurements of the chunk: [Tc][ny] shared, or [Tc][F][ny] (y_per = 1)
    const double* zero_u;    // MAXU zeros: the u of a model without inputs
    double *ll, *x, *xt, *R, *Rt, *e;   // per-step outputs of the chunk, each optional: [Tc][F], [Tc][F][nx], [Tc][F][nx][nx], [Tc][F][ny]
    int64_t F;
    int64_t t0;              // first step of this chunk
    int32_t Tc, nu;
    int32_t u_per, y_per;
    int32_t first;           // 1: the first chunk of a run (ll_total starts at 0)
    int32_t pad;
    double t_index0, Ts;     // tau_t = (t_index0 + t) * Ts, as llpf_run and k_simulate take it
    double gamma, wm0, wc0, wi;   // the sigma-point spread and weights of the bank (llpf_ukf_weights)
    double* post;            // optional [Tc][nx + np][F]: the posterior xt, packed Rt of every step, SoA (what k_ukf_smooth reads);
                             // null: k_ukf<..., false>, the kernel of a run
};
// arguments of k_ukf_smooth: one launch is the backward pass over one chunk of steps [t0, t0 + Tc), run from t0 + Tc - 1 down to t0, one
// thread per filter
struct UkfSmoothArgs {
    const double* par;       // [np(nx) + np(ny)][F] as UkfArgs::par (R1 is read)
    const double* post;      // [Tc][nx + np][F] the posterior of the chunk's steps (UkfArgs::post of the forward pass)
    double* carry;           // [nx + np][F] xT, packed RT: in, those of step t0 + Tc (unless init); out, those of step t0
    const double* u;         // inputs of the chunk: [Tc][nu] shared, or [Tc][F][nu] (u_per = 1); unused when nu = 0
    const double* zero_u;    // MAXU zeros: the u of a model without inputs
    double *xT, *RT;         // per-step outputs of the chunk, each optional: [Tc][F][nx], [Tc][F][nx][nx]
    int64_t F;
    int64_t t0;              // first step of this chunk
    int32_t Tc, nu;
    int32_t u_per;
    int32_t init;            // 1: the chunk holds the run's last step, where xT = xt, RT = Rt (the carry is not read)
    double t_index0, Ts;     // tau_t = (t_index0 + t) * Ts, the forward pass's
    double gamma, wm0, wc0, wi;
};
