// k_sqkf.hip — k_sqkf (kernels/sqkf.hpp): banks of square-root Kalman filters with constant matrices (llpf_sqkf_bank_run).
// One of the engine's device translation units: every (NX, NY) of 1..8 x 1..4 is instantiated here and nowhere else, by dispatch_dim
// (kernels/dispatch.hpp).
#include "engine.hpp"
#include "shared/llpf_sqkf.h"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/kf_store.hpp"
#include "kernels/sqkf.hpp"
#include "kernels/dispatch.hpp"
#include "kernels/jit_bank.hpp"      // kf_grid

template <int NX, int NY>
static hipError_t launch_sqkf_t(const KalmanArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((k_sqkf<NX, NY>), kf_grid(a.F), dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_sqkf(int nx, int ny, const KalmanArgs& a, hipStream_t s) {
    return dispatch_dim<1, 8>(nx, [&](auto NX) { return dispatch_dim<1, 4>(ny, [&](auto NY) { return launch_sqkf_t<decltype(NX)::value, decltype(NY)::value>(a, s); }); });
}

}  // namespace llpf
