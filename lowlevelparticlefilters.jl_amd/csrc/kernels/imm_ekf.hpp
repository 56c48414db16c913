// kernels/imm_ekf.hpp — k_imm_ekf: banks of interacting-multiple-model filters whose modes are first-order extended Kalman filters of one
// model type (llpf_imm_bank_run_at on a bank with LLPF_IMM_EXTENDED; host side: host/imm.hpp).  Part of k_imm_ekf.hip (namespace llpf,
// after kernels/imm.hpp), and the text of the run-time program of a user model's kernel (jit_imm_ekf.inc).
// ------------------------------------------------------------------------------------------------
// The step, the exchange between the modes and their rules are kernels/imm.hpp's imm_chunk; here is the mode.  Its own step is
// shared/llpf_ekf.h with literal NX, NY around Model::measurement_jac (stage 2, at the mode's prior; a missing row: skipped, ll_j = 0)
// and Model::dynamics_jac (stage 6, at the mode's x after the mixing), as k_ekf runs it: value, Jacobian and the temporaries are local
// arrays.  The model reads the lane's own descriptor ModelD[f * G + j], prepared at the step's tau; R1, R2 come from the SoA
// [entry][F * G].  A lane's bits are those of the host loop over the two shared headers.
// An idle lane reads mode 0's column — descriptor, R1, R2 and state — so that the model never sees a zero descriptor (a zero divisor, a
// zero supersample).
// ------------------------------------------------------------------------------------------------
template <class Model, int NX, int NY>
struct ImmEkfMode {
    static constexpr bool IDLE_ON_MODE0 = true;
    const ModelD* __restrict__ models;
    const ImmEkfArgs& a;
    Model model;
    DEV ImmEkfMode(const ModelD* models_, const ImmEkfArgs& a_) : models(models_), a(a_) {}
    DEV int npar(int) const { return LLPF_EKF_NPAR(NX, NY); }
    DEV const double* no_u() const { return a.zero_u; }
    DEV const double* begin(const double* P, int64_t col, const double* u, int k) {
        model.prepare(models + col, u, (a.t_index0 + (double)(a.t0 + k)) * a.Ts);
        return P;
    }
    DEV bool missing(const double* y) const { return llpf_ekf_missing(y); }
    DEV double correct(const double* P, int64_t L, const double*, const double* y, bool missing, double* x, double* R) {
        if (missing) return 0.0;
        double gx[NY], C[NY * NX], yr[NY], e[NY];
        model.measurement_jac(x, gx, C);
#pragma unroll
        for (int r = 0; r < NY; ++r) yr[r] = y[r];
        return llpf_ekf_correct(NX, NY, P, L, yr, gx, C, NX, x, R, e);
    }
    DEV void predict(const double* P, int64_t L, const double*, double* x, double* R) {
        double fx[NX], A[NX * NX];
        model.dynamics_jac(x, fx, A);
        llpf_ekf_predict(NX, P, L, fx, A, NX, x, R);
    }
};

template <class Model, int NX, int NY, int G>
__global__ __launch_bounds__(KF_BLOCK) void k_imm_ekf(const ModelD* __restrict__ models, ImmEkfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no extended Kalman filter");
    static_assert(has_dynamics_jac<Model>::value, "an extended Kalman filter needs Model::dynamics_jac(x, fx, J)");
    static_assert(has_measurement_jac<Model>::value, "an extended Kalman filter needs Model::measurement_jac(x, gx, J)");
    ImmEkfMode<Model, NX, NY> mode{models, a};
    imm_chunk<NX, NY, G>(a, mode);
}
