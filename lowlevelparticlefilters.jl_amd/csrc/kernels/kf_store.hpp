// kernels/kf_store.hpp — what the one-thread-per-filter kernels share (k_kalman, k_kalman_smooth: kernels/kalman.hpp; k_ukf: kernels/ukf.hpp):
// the workgroup size and the stores of a lane's consecutive doubles into the time-major outputs [Tc][F][...].  Included inside namespace
// llpf, and part of the run-time program of a model's k_ukf (jit_ukf.inc).
constexpr int KF_BLOCK = 64;      // one wave per workgroup: a bank of 10^3 filters still spreads over 16 CUs

typedef double llpf_kf_d2 __attribute__((ext_vector_type(2)));
template <int N>
DEV void kf_store(double* p, const double* v) {
    if constexpr (N % 2 == 0) {       // 16-byte stores: p is 16-byte aligned (N even, the buffer 256-byte aligned)
#pragma unroll
        for (int d = 0; d < N; d += 2) {
            llpf_kf_d2 w;
            w.x = v[d];
            w.y = v[d + 1];
            *reinterpret_cast<llpf_kf_d2*>(p + d) = w;
        }
    } else {
#pragma unroll
        for (int d = 0; d < N; ++d) p[d] = v[d];
    }
}
// the dense nx x nx form of the packed R, row by row
template <int NX>
DEV void kf_store_dense(double* p, const double* R) {
    double row[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
#pragma unroll
        for (int c = 0; c < NX; ++c) row[c] = R[llpf_kf_idx(r, c)];
        kf_store<NX>(p + r * NX, row);
    }
}

