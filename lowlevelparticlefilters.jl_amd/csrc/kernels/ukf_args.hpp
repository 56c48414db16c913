// kernels/ukf_args.hpp — arguments of k_ukf and k_ukf_smooth (kernels/ukf.hpp).  Included inside namespace llpf by engine.hpp (host side)
// and compiled into the run-time programs of a model's k_ukf and k_ukf_smooth (k_ukf.hip, jit_ukf.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of F unscented Kalman filters (kernels/kf_model_args.hpp), one thread per filter.
struct UkfArgs : KfModelArgs {
    double gamma, wm0, wc0, wi;   // the sigma-point spread and weights of the bank (llpf_ukf_weights)
    double* post;            // optional [Tc][nx + np][F]: the posterior xt, packed Rt of every step, SoA (what k_ukf_smooth reads);
                             // null: k_ukf<..., false>, the kernel of a run
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"      // a struct with a base and members of its own: clang computes it, and warns
static_assert(sizeof(UkfArgs) == 184 && __builtin_offsetof(UkfArgs, gamma) == 144, "kernel argument layout");
#pragma clang diagnostic pop
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
