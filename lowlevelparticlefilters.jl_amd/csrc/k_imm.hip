// k_imm.hip — k_imm (kernels/imm.hpp: the step frame imm_chunk with ImmKalmanMode): banks of interacting-multiple-model filters over
// Kalman filters with constant matrices (llpf_imm_bank_run).  No model code is instantiated here.
// One of the engine's device translation units: every (NX, NY, G) of 1..8 x 1..4 x {1, 2, 4} is instantiated here and nowhere else, by
// dispatch_dim (kernels/dispatch.hpp).
#include "engine.hpp"
#include "shared/llpf_imm.h"

namespace llpf {

#define DEV __device__ __forceinline__

#include "kernels/imm_args.hpp"
#include "kernels/kf_store.hpp"
#include "kernels/imm.hpp"
#include "kernels/dispatch.hpp"

template <int NX, int NY, int G>
static hipError_t launch_imm_t(const ImmArgs& a, hipStream_t s) {
    const int64_t L = a.F * G;
    hipLaunchKernelGGL((k_imm<NX, NY, G>), dim3((unsigned)((L + KF_BLOCK - 1) / KF_BLOCK), 1, 1), dim3(KF_BLOCK), 0, s, a);
    return hipGetLastError();
}
// g: the lanes per filter, 1, 2 or 4 (imm_group)
hipError_t launch_imm(int nx, int ny, int g, const ImmArgs& a, hipStream_t s) {
    if (g != 1 && g != 2 && g != 4) return hipErrorInvalidValue;
    return dispatch_dim<1, 8>(nx, [&](auto NX) {
        return dispatch_dim<1, 4>(ny, [&](auto NY) {
            constexpr int X = decltype(NX)::value, Y = decltype(NY)::value;
            return g == 1 ? launch_imm_t<X, Y, 1>(a, s) : g == 2 ? launch_imm_t<X, Y, 2>(a, s) : launch_imm_t<X, Y, 4>(a, s);
        });
    });
}

}  // namespace llpf
