// kernels/ekf_args.hpp — arguments of k_ekf (kernels/ekf.hpp).  Included inside namespace llpf by engine.hpp (host side) and compiled into
// the run-time program of a model's k_ekf (k_ekf.hip, jit_ekf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F extended Kalman filters, one thread per filter.  Device arrays are SoA / time-major
// as k_kalman's: a wave's 64 lanes read and write whole lines.
struct EkfArgs {
    static constexpr bool ITERATED = false;
    const double* par;       // [np(nx) + np(ny)][F] R1, R2 as packed lower triangles (shared/llpf_ekf.h: LLPF_EKF_OFF_*)
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
// ... and of its iterated form, k_ekf<Model, NX, NY, IekfArgs>: the same chunk with the iteration of correct! (shared/llpf_ekf.h)
struct IekfArgs : EkfArgs {
    static constexpr bool ITERATED = true;
    int32_t maxiters, pad2;  // 2..LLPF_IEKF_MAXITERS linearisations of a step's measurement at most
    double epsilon;          // >= 0: the step is over once no state moved by more than this
};
