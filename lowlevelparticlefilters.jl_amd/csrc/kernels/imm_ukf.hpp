// kernels/imm_ukf.hpp — k_imm_ukf: banks of interacting-multiple-model filters whose modes are unscented Kalman filters of one model type
// (llpf_imm_bank_run_at on a bank of llpf_imm_bank_create_unscented; host side: host/imm.hpp).  Part of k_imm_ukf.hip (namespace llpf,
// after kernels/ukf.hpp and kernels/imm.hpp), and the text of the run-time program of a user model's kernel (jit_imm_ukf.inc).
// ------------------------------------------------------------------------------------------------
// The step, the exchange between the modes and their rules are kernels/imm.hpp's imm_chunk; here is the mode.  Its own step is
// shared/llpf_ukf.h with literal NX, NY around Model::measurement (stage 2, the 2 NX + 1 points of the mode's prior; a missing row:
// skipped, ll_j = 0) and Model::dynamics (stage 6, the points of the mode's x, R after the mixing), operation for operation what k_ukf
// runs between its model.prepare and its stores: factor, one evaluation per point into Z, finish.  The model needs no Jacobian members.
// The model reads the lane's own descriptor ModelD[f * G + j], prepared at the step's tau; R1, R2 come from the SoA [entry][F * G]; the
// weights ride in the launch arguments, one set per bank.  A lane's bits are those of the host loop over the two shared headers.
// Where the mapped points live is k_ukf's rule (kernels/ukf.hpp: UKF_POINTS_LDS): up to NX = 4 a local array of the mode, from NX = 5
// [point][d][lane] in LDS, lane fastest (conflict-free 8-byte accesses), declared by the kernel, which hands the mode its lane's pointer;
// the stride between a lane's entries, the KF_BLOCK lanes of the workgroup, is the mode's constant ZS, which sizes the kernel's array
// (ZLEN) as well: a constant, so that the indices of the local array are literals and it lives in registers.  Every lane of the
// workgroup owns its slot — an idle lane and a lane past L as well — and no lane touches another's: no barrier.
// An idle lane reads mode 0's column — descriptor, R1, R2 and state — so that the model never sees a zero descriptor.
// A mode whose R (either factorisation) or S loses definiteness is NaN from there (shared/llpf_ukf.h); its ll_j is NaN and stage 3 makes
// the whole IMM NaN (llpf_imm_poison): these branches are per lane and stay inside correct / predict (kernels/imm.hpp: fetch uniformity).
// ------------------------------------------------------------------------------------------------
template <class Model, int NX, int NY>
struct ImmUkfMode {
    static constexpr bool IDLE_ON_MODE0 = true;
    static constexpr int NP = LLPF_KF_NP(NX), NPT = LLPF_UKF_NPTS(NX), ZD = NX > NY ? NX : NY;
    static constexpr bool LDS = UKF_POINTS_LDS(NX, NY);
    static constexpr int64_t ZS = LDS ? KF_BLOCK : 1;               // the stride of a lane's entries of Z
    static constexpr int ZLEN = LDS ? NPT * ZD * KF_BLOCK : 1;      // the kernel's LDS array, doubles
    const ModelD* __restrict__ models;
    const ImmUkfArgs& a;
    Model model;
    double* zl;                       // LDS: this lane's slot of the kernel's array (stride ZS)
    double zreg[LDS ? 1 : NPT * ZD];
    DEV ImmUkfMode(const ModelD* models_, const ImmUkfArgs& a_, double* zl_) : models(models_), a(a_), zl(zl_) {}
    DEV int npar(int) const { return LLPF_UKF_NPAR(NX, NY); }
    DEV const double* no_u() const { return a.zero_u; }
    DEV const double* begin(const double* P, int64_t col, const double* u, int k) {
        model.prepare(models + col, u, (a.t_index0 + (double)(a.t0 + k)) * a.Ts);
        return P;
    }
    DEV bool missing(const double* y) const { return !(y[0] == y[0]); }
    DEV double correct(const double* P, int64_t L, const double*, const double* y, bool missing, double* x, double* R) {
        if (missing) return 0.0;
        double* Z = LDS ? zl : zreg;
        double e[NY], Cf[NP];
        const int ok = llpf_ukf_factor(NX, R, Cf);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            double X[NX], Y[NY];
            llpf_ukf_point(NX, a.gamma, x, Cf, i, X);
            model.measurement(X, Y);
#pragma unroll
            for (int r = 0; r < NY; ++r) Z[(i * NY + r) * ZS] = Y[r];
        }
        double yr[NY];
#pragma unroll
        for (int r = 0; r < NY; ++r) yr[r] = y[r];
        return llpf_ukf_correct_finish(NX, NY, a.gamma, a.wm0, a.wc0, a.wi, P, L, ok, Cf, Z, ZS, yr, x, R, e);
    }
    DEV void predict(const double* P, int64_t L, const double*, double* x, double* R) {
        double* Z = LDS ? zl : zreg;
        double Cf[NP];
        const int ok = llpf_ukf_factor(NX, R, Cf);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            double X[NX], Xn[NX];
            llpf_ukf_point(NX, a.gamma, x, Cf, i, X);
            model.dynamics(X, Xn);
#pragma unroll
            for (int d = 0; d < NX; ++d) Z[(i * NX + d) * ZS] = Xn[d];
        }
        llpf_ukf_predict_finish(NX, a.wm0, a.wc0, a.wi, P, L, ok, Z, ZS, x, R);
    }
};

template <class Model, int NX, int NY, int G>
__global__ __launch_bounds__(KF_BLOCK) void k_imm_ukf(const ModelD* __restrict__ models, ImmUkfArgs a) {
    static_assert(!Model::RB, "the Rao-Blackwellized models have no unscented filter");
    using Mode = ImmUkfMode<Model, NX, NY>;
    __shared__ double zsh[Mode::ZLEN];
    Mode mode{models, a, zsh + threadIdx.x};
    imm_chunk<NX, NY, G>(a, mode);
}
