// k_kalman.hip — k_kalman, k_kalman_smooth (kernels/kalman.hpp): banks of Kalman filters with constant matrices (llpf_kalman_bank_run,
// llpf_kalman_bank_smooth).
// One of the engine's device translation units: every (NX, NY) of 1..8 x 1..4 (k_kalman) and every NX of 1..8 (k_kalman_smooth) is
// instantiated here and nowhere else, by dispatch_dim (kernels/dispatch.hpp).
#include "engine.hpp"
#include "shared/llpf_kalman.h"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/kf_store.hpp"
#include "kernels/kalman.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"      // kf_grid

template <int NX, int NY>
static hipError_t launch_kalman_t(const KalmanArgs& a, hipStream_t s) {
    if (a.post)
        hipLaunchKernelGGL((k_kalman<NX, NY, true>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((k_kalman<NX, NY, false>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_kalman(int nx, int ny, const KalmanArgs& a, hipStream_t s) {
    return dispatch_dim<1, 8>(nx, [&](auto NX) { return dispatch_dim<1, 4>(ny, [&](auto NY) { return launch_kalman_t<decltype(NX)::value, decltype(NY)::value>(a, s); }); });
}

template <int NX>
static hipError_t launch_kalman_smooth_t(const KalmanSmoothArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_kalman_smooth<NX>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_kalman_smooth(int nx, const KalmanSmoothArgs& a, hipStream_t s) {
    return dispatch_dim<1, 8>(nx, [&](auto NX) { return launch_kalman_smooth_t<decltype(NX)::value>(a, s); });
}

}  // namespace llpf
