// kernels/ekf_args.hpp — arguments of k_ekf (kernels/ekf.hpp).  Included inside namespace llpf by engine.hpp (host side) and compiled into
// the run-time program of a model's k_ekf (k_ekf.hip, jit_ekf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F extended Kalman filters (kernels/kf_model_args.hpp), one thread per filter: the
// plain filter has no argument of its own.
struct EkfArgs : KfModelArgs {
    static constexpr bool ITERATED = false;
};
// ... and of its iterated form, k_ekf<Model, NX, NY, IekfArgs>: the same chunk with the iteration of correct! (shared/llpf_ekf.h)
struct IekfArgs : EkfArgs {
    static constexpr bool ITERATED = true;
    int32_t maxiters, pad2;  // 2..LLPF_IEKF_MAXITERS linearisations of a step's measurement at most
    double epsilon;          // >= 0: the step is over once no state moved by more than this
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"      // a struct with a base and members of its own: clang computes it, and warns
static_assert(sizeof(EkfArgs) == 144 && sizeof(IekfArgs) == 160 && __builtin_offsetof(IekfArgs, maxiters) == 144, "kernel argument layout");
#pragma clang diagnostic pop
