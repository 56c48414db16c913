// k_kalman.hip — k_kalman, k_kalman_smooth (kernels/kalman.hpp): banks of Kalman filters with constant matrices (llpf_kalman_bank_run,
// llpf_kalman_bank_smooth).
// One of the engine's device translation units: every (NX, NY) of 1..8 x 1..4 (k_kalman) and every NX of 1..8 (k_kalman_smooth) is
// instantiated here and nowhere else.
#include "engine.hpp"
#include "shared/llpf_kalman.h"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/kf_store.hpp"
#include "kernels/kalman.hpp"

template <int NX, int NY>
static hipError_t launch_kalman_t(const KalmanArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1);
    if (a.post)
        hipLaunchKernelGGL((k_kalman<NX, NY, true>), g, dim3(KF_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((k_kalman<NX, NY, false>), g, dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}
template <int NX>
static hipError_t launch_kalman_nx(int ny, const KalmanArgs& a, hipStream_t s) {
    switch (ny) {
        case 1: return launch_kalman_t<NX, 1>(a, s);
        case 2: return launch_kalman_t<NX, 2>(a, s);
        case 3: return launch_kalman_t<NX, 3>(a, s);
        case 4: return launch_kalman_t<NX, 4>(a, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_kalman(int nx, int ny, const KalmanArgs& a, hipStream_t s) {
    switch (nx) {
        case 1: return launch_kalman_nx<1>(ny, a, s);
        case 2: return launch_kalman_nx<2>(ny, a, s);
        case 3: return launch_kalman_nx<3>(ny, a, s);
        case 4: return launch_kalman_nx<4>(ny, a, s);
        case 5: return launch_kalman_nx<5>(ny, a, s);
        case 6: return launch_kalman_nx<6>(ny, a, s);
        case 7: return launch_kalman_nx<7>(ny, a, s);
        case 8: return launch_kalman_nx<8>(ny, a, s);
        default: return hipErrorInvalidValue;
    }
}

template <int NX>
static hipError_t launch_kalman_smooth_t(const KalmanSmoothArgs& a, hipStream_t s) {
    const dim3 g((unsigned)((a.F + KF_BLOCK - 1) / KF_BLOCK), 1, 1);
    hipLaunchKernelGGL((k_kalman_smooth<NX>), g, dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_kalman_smooth(int nx, const KalmanSmoothArgs& a, hipStream_t s) {
    switch (nx) {
        case 1: return launch_kalman_smooth_t<1>(a, s);
        case 2: return launch_kalman_smooth_t<2>(a, s);
        case 3: return launch_kalman_smooth_t<3>(a, s);
        case 4: return launch_kalman_smooth_t<4>(a, s);
        case 5: return launch_kalman_smooth_t<5>(a, s);
        case 6: return launch_kalman_smooth_t<6>(a, s);
        case 7: return launch_kalman_smooth_t<7>(a, s);
        case 8: return launch_kalman_smooth_t<8>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace llpf
