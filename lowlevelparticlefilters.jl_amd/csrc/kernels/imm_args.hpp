// kernels/imm_args.hpp — arguments of k_imm (kernels/imm.hpp), of k_imm_ekf (kernels/imm_ekf.hpp) and of k_imm_ukf (kernels/imm_ukf.hpp),
// and k_imm's launcher.  Included inside namespace llpf by the units that know the IMM banks: k_imm.hip, k_imm_ekf.hip, k_imm_ukf.hip
// and, through host/imm.hpp, capi.hip (the host side); compiled into the run-time programs of a model's k_imm_ekf and k_imm_ukf
// (jit_imm_ekf.inc, jit_imm_ukf.inc: tools/gen_jit_prelude.py drops the launcher's declaration from that text).
// One launch is one chunk of steps [t0, t0 + Tc) of F IMM filters of M modes, one lane per (filter, mode): G = 1, 2 or 4 lanes per filter
// (the smallest G >= M), thread f * G + j is mode j of filter f, the lanes j >= M idle.  L = F * G is the number of columns of the SoA
// arrays: a lane's column is its thread index.
// What the step frame reads (kernels/imm.hpp: imm_chunk): the leading members of both kernels' arguments
struct ImmBaseArgs {
    const double* par;       // [npar + LLPF_IMM_MAXM][L]: the mode's own constants (npar rows), then column j of the filter's transition
                             // matrix, P_ij at row npar + i
    double* state;           // [nx + np + 2][L] the mode's x, packed R and mu_j, the run's running ll_total: in at t0, out at t0 + Tc
    const double* u;         // inputs of the chunk: [Tc][nu] shared, or [Tc][F][nu] (u_per = 1); unused when nu = 0
    const double* y;         // measurements of the chunk: [Tc][ny] shared, or [Tc][F][ny] (y_per = 1)
    double *ll, *x, *xt, *R, *Rt;   // per-step outputs of the chunk, each optional: [Tc][F], [Tc][F][nx], [Tc][F][nx][nx] (the combined estimate)
    double *mu, *ll_modes;   // ... and [Tc][F][M]: the posterior mode probabilities, every mode's own ll
    int64_t F;
    int32_t Tc, nu, M;
    int32_t u_per, y_per;
    int32_t first;           // 1: the first chunk of a run (ll_total starts at 0)
    int32_t interact;        // 1: the modes mix after every step
    int32_t pad;
};
// Kalman modes: par holds the constant matrices (shared/llpf_kalman.h: LLPF_KF_OFF_*)
struct ImmArgs : ImmBaseArgs {
    int64_t par_tstride;     // always 0 (kernels/kalman.hpp: KF_RELOAD)
};
// extended Kalman modes of one model type: par holds R1, R2 as packed lower triangles (shared/llpf_ekf.h: LLPF_EKF_OFF_*)
struct ImmEkfArgs : ImmBaseArgs {
    const double* zero_u;    // MAXU zeros: the u of a model without inputs
    int64_t t0;              // first step of this chunk
    double t_index0, Ts;     // tau_t = (t_index0 + t) * Ts, as k_ekf takes it
};
// unscented Kalman modes of one model type: par and the time as for the extended modes (R1, R2 packed: shared/llpf_ukf.h: LLPF_UKF_OFF_*)
struct ImmUkfArgs : ImmEkfArgs {
    double gamma, wm0, wc0, wi;   // the sigma-point spread and weights of the bank (llpf_ukf_weights), as in UkfArgs
};
static_assert(sizeof(ImmBaseArgs) == 128 && sizeof(ImmArgs) == 136 && sizeof(ImmEkfArgs) == 160 && sizeof(ImmUkfArgs) == 192,
              "kernel argument layout");
// one chunk of steps (k_imm.hip): nx in 1..8, ny in 1..4, g = 1, 2 or 4 lanes per filter (the smallest g >= ImmArgs::M)
hipError_t launch_imm(int nx, int ny, int g, const ImmArgs& a, hipStream_t s);
