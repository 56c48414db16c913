// kernels/dispatch.hpp — from run-time dimensions and model ids to the template arguments of a launcher (host side; part of every unit
// that instantiates kernels by dimension or by built-in model, namespace llpf).
// ------------------------------------------------------------------------------------------------
// The callable is a generic lambda; what it instantiates is what the unit holds: the precompiled set of a kernel is the range its
// launcher dispatches over, and nothing else (tests/test_kernel_symbols.py).

// f(std::integral_constant<int, N>{}) for N == n in LO..HI
template <int LO, int HI, class F>
static hipError_t dispatch_dim(int n, F&& f) {
    if constexpr (LO > HI) return hipErrorInvalidValue;
    else return n == LO ? f(std::integral_constant<int, LO>{}) : dispatch_dim<LO + 1, HI>(n, f);
}

template <int NX, int NY> struct LinGauss;      // kernels/models.hpp
template <int NX, int NY> struct QuadTank;
template <class M, int NX_, int NY_>
struct ModelTag {
    using Model = M;
    static constexpr int NX = NX_, NY = NY_;
};

// f(ModelTag<LinGauss<nx, ny>, nx, ny>{}) for nx, ny in 1..4: the precompiled linear-Gaussian shapes (above them: jit_builtin_lg)
template <class F>
static hipError_t dispatch_lingauss(int nx, int ny, F&& f) {
    return dispatch_dim<1, 4>(nx, [&](auto NX) {
        return dispatch_dim<1, 4>(ny, [&](auto NY) { return f(ModelTag<LinGauss<decltype(NX)::value, decltype(NY)::value>, decltype(NX)::value, decltype(NY)::value>{}); });
    });
}
// the models with precompiled kernels: LLPF_MODEL_LINEAR_GAUSSIAN as above, LLPF_MODEL_QUADTANK_RK4 as QuadTank<4, 2> at (4, 2) only
template <class F>
static hipError_t dispatch_builtin_model(int model_id, int nx, int ny, F&& f) {
    if (model_id == LLPF_MODEL_QUADTANK_RK4) return nx == 4 && ny == 2 ? f(ModelTag<QuadTank<4, 2>, 4, 2>{}) : hipErrorInvalidValue;
    if (model_id == LLPF_MODEL_LINEAR_GAUSSIAN) return dispatch_lingauss(nx, ny, f);
    return hipErrorInvalidValue;
}
