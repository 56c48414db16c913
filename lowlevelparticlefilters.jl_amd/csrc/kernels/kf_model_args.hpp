// kernels/kf_model_args.hpp — the arguments that the kernels of the model-driven Kalman banks have in common: the leading members of
// UkfArgs (kernels/ukf_args.hpp) and of EkfArgs (kernels/ekf_args.hpp).  Included inside namespace llpf by engine.hpp (host side) and
// compiled into the run-time programs of a model's k_ukf and k_ekf (jit_ukf.inc, jit_ekf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F filters, one thread per filter.  Device arrays are SoA / time-major as k_kalman's:
// a wave's 64 lanes read and write whole lines.
struct KfModelArgs {
    const double* par;       // [np(nx) + np(ny)][F] R1, R2 as packed lower triangles (shared/llpf_ukf.h: LLPF_UKF_OFF_*, llpf_ekf.h: LLPF_EKF_OFF_*)
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
};
// the kernels take UkfArgs, EkfArgs and IekfArgs by value: with this base their bytes are what they were with the members spelled out
static_assert(sizeof(KfModelArgs) == 144, "kernel argument layout");
