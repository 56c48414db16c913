// kernels/imm_ekf_args.hpp — arguments of k_imm_ekf (kernels/imm_ekf.hpp).  Included inside namespace llpf by the two units that know the
// extended IMM bank: k_imm_ekf.hip (the kernel) and, through host/imm.hpp, capi.hip (the host side), and compiled into the run-time program
// of a model's k_imm_ekf (jit_imm_ekf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F IMM filters of M modes, every mode a first-order extended Kalman filter of one model
// type; lanes, groups and columns are those of kernels/imm_args.hpp (G lanes per filter, L = F * G columns, thread f * G + j is mode j).
struct ImmEkfArgs {
    const double* par;       // [LLPF_EKF_NPAR(nx, ny) + LLPF_IMM_MAXM][L]: the mode's R1, R2 as packed lower triangles (shared/llpf_ekf.h:
                             // LLPF_EKF_OFF_*), then column j of the filter's transition matrix, P_ij at row npar + i
    double* state;           // [nx + np + 2][L] the mode's x, packed R and mu_j, the run's running ll_total: in at t0, out at t0 + Tc
    const double* u;         // inputs of the chunk: [Tc][nu] shared, or [Tc][F][nu] (u_per = 1); unused when nu = 0
    const double* y;         // measurements of the chunk: [Tc][ny] shared, or [Tc][F][ny] (y_per = 1)
    const double* zero_u;    // MAXU zeros: the u of a model without inputs
    double *ll, *x, *xt, *R, *Rt;   // per-step outputs of the chunk, each optional: [Tc][F], [Tc][F][nx], [Tc][F][nx][nx] (the combined estimate)
    double *mu, *ll_modes;   // ... and [Tc][F][M]: the posterior mode probabilities, every mode's own ll
    int64_t F;
    int64_t t0;              // first step of this chunk
    int32_t Tc, nu, M;
    int32_t u_per, y_per;
    int32_t first;           // 1: the first chunk of a run (ll_total starts at 0)
    int32_t interact;        // 1: the modes mix after every step
    int32_t pad;
    double t_index0, Ts;     // tau_t = (t_index0 + t) * Ts, as k_ekf takes it
};
static_assert(sizeof(ImmEkfArgs) == 160, "kernel argument layout");
