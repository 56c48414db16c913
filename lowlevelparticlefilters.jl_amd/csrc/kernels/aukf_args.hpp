// kernels/aukf_args.hpp — arguments of k_aukf (kernels/aukf.hpp).  Included inside namespace llpf by engine.hpp (host side) and compiled
// into the run-time programs of a model's k_aukf (k_aukf.hip, jit_aukf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F augmented unscented Kalman filters (kernels/kf_model_args.hpp), one thread per filter.
struct AukfArgs : KfModelArgs {
    double gamma, wm0, wc0, wi;       // the measurement set: the points of correct!, L = nx (llpf_ukf_weights)
    double gamma_a, wm0a, wc0a, wia;  // the dynamics set: the points of predict! over (x; w), L = 2 nx
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"      // a struct with a base and members of its own: clang computes it, and warns
static_assert(sizeof(AukfArgs) == 208 && __builtin_offsetof(AukfArgs, gamma) == 144, "kernel argument layout");
#pragma clang diagnostic pop
