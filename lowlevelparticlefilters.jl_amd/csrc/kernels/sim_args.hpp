// kernels/sim_args.hpp — arguments of k_simulate (kernels/simulate.hpp).  Included inside namespace llpf by engine.hpp (host side) and
// compiled into the run-time program of a user model's k_simulate (k_simulate.hip, jit_simulate.inc).
// One launch is one chunk of steps [t0, t0 + Tc) of M trajectories of each of F filters (grid: trajectory tiles x filters).
struct SimArgs {
    const double* u;         // inputs of the chunk: u_t of (filter f, trajectory m) at u + f * u_fstride + m * u_mstride + (t - t0) * nu
    int64_t u_fstride, u_mstride;   //   (both 0: one input sequence shared by every trajectory)
    double* X;               // [F][Tc][M][nx] states x_t of the chunk, or nullptr
    double* Y;               // [F][Tc][M][ny] measurements y_t of the chunk, or nullptr
    double* xs;              // [F][nx][M] the state carried from one chunk to the next (x_{t0} in, x_{t0 + Tc} out)
    const double* zero_u;    // MAXU zeros: the u a model's initial density sees (k_init_user) and the u of a model without inputs
    int64_t M;               // trajectories per filter
    int64_t T;               // steps of the whole simulation (no propagation after the last)
    int64_t t0;              // first step of this chunk
    int32_t Tc;              // steps of this chunk
    int32_t nu;
    int32_t flags;           // LLPF_SIM_* of include/llpf.h
    int32_t nt;              // 1: nontemporal stores of X / Y (a chunk's output larger than the Infinity Cache)
    uint32_t step0;          // Philox step of t = 0 (initial draw at step0, step t at step0 + t)
    uint32_t pad;
    double t_index0, Ts;     // tau_t = (t_index0 + t) * Ts, as llpf_run takes it
    uint64_t key0, key_stride;   // Philox key of filter f: key0 + f * key_stride (as set_keys derives a filter's own key)
};
