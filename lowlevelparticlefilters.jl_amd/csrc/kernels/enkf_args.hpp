// kernels/enkf_args.hpp — arguments of k_enkf and k_enkf_init (kernels/enkf.hpp).  Included inside namespace llpf by engine.hpp (host side)
// and compiled into the run-time program of a model's k_enkf (k_enkf.hip, jit_enkf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F ensemble Kalman filters (kernels/kf_model_args.hpp), one workgroup per filter.
// KfModelArgs::state is [nx + np + 1][F]: the ensemble mean, its packed sample covariance and the running ll_total, written at the end
// of the chunk; par is the unscented bank's block (R1, R2 packed), of which R2 is read.
struct EnkfArgs : KfModelArgs {
    double* members;         // [F][nx][N] the ensembles, SoA: member i of a lane is consecutive with its neighbours'
    uint64_t key0;           // filter f's Philox key is key0 + f
    double rho;              // inflation (1: none)
    int32_t N;               // members per ensemble, 2..LLPF_ENKF_MAX_MEMBERS
    uint32_t step0;          // Philox step of the run's first step: step t of the run draws at step0 + t
    int32_t phases;          // LLPF_ENKF_CORRECT | LLPF_ENKF_PREDICT: what a step runs (the step verbs run one of them)
    int32_t pad2;
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(EnkfArgs) == 184 && __builtin_offsetof(EnkfArgs, members) == 144, "kernel argument layout");
#pragma clang diagnostic pop
// arguments of k_enkf_init: reset! of every ensemble
struct EnkfInitArgs {
    double* members;         // [F][nx][N]
    const double* zero_u;    // MAXU zeros: prepare() of a model with an initial density of its own sees u = 0
    uint64_t key0;
    int32_t N;
    uint32_t n_reset;        // the counter of the draw
};
