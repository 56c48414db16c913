// host/simulate.hpp — simulate(pf, T, du) for M trajectories at once (llpf_simulate / llpf_bank_simulate; kernel: kernels/simulate.hpp).
// Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The steps run through the chunked staging pipeline of host/pipe.hpp, which counts the bytes of one step's outputs: a chunk's outputs
// fit a 64 MiB staging buffer unless a single step is larger.  The state x carries from chunk to chunk in a device buffer [F][nx][M], so a
// long run's prefix is a short run, bit for bit.  Outputs of a chunk beyond the Infinity Cache are stored nontemporal.
constexpr size_t SIM_INFINITY_CACHE = (size_t)256 << 20;

static int bank_simulate(Bank& b, int64_t M, int64_t T, const double* U, int32_t u_per_traj, double t_index0, uint64_t seed, uint32_t step0,
                         int32_t flags, double* X, double* Y) {
    if (M < 1) return fail(LLPF_ERR_ARG, "simulate: M must be >= 1");
    if (M > INT32_MAX) return fail(LLPF_ERR_ARG, "simulate: M must be below 2^31 (a trajectory's Philox counter is 32 bits)");
    if (T < 1) return fail(LLPF_ERR_ARG, "simulate: T must be >= 1");
    if (!X && !Y) return fail(LLPF_ERR_ARG, "simulate: X and Y are both null");
    if (flags & ~(LLPF_SIM_DYNAMICS_NOISE | LLPF_SIM_MEASUREMENT_NOISE | LLPF_SIM_SAMPLE_INITIAL)) return fail(LLPF_ERR_ARG, "simulate: unknown flag bits");
    if (u_per_traj != 0 && u_per_traj != 1) return fail(LLPF_ERR_ARG, "simulate: u_per_trajectory must be 0 or 1");
    const int model_id = b.cfg.model.model_id;
    if (model_id == LLPF_MODEL_RB_LINEAR || model_id == LLPF_MODEL_RB_BILINEAR)
        return fail(LLPF_ERR_ARG, "simulate: the Rao-Blackwellized models (LLPF_MODEL_RB_LINEAR, LLPF_MODEL_RB_BILINEAR) are not simulated");
    if (b.nu > 0 && !U) return fail(LLPF_ERR_ARG, "simulate: U is null");
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu;
    // every size product checked: the caller's arrays are F * T * M * (nx | ny) doubles, U F * M * T * nu
    const uint64_t w = (uint64_t)(X ? nx : 0) + (uint64_t)(Y ? ny : 0), FM = (uint64_t)F * (uint64_t)M;
    uint64_t total = 0, ud = 0;
    if (!doubles_fit({FM, w, (uint64_t)T}, total) || !doubles_fit({FM, (uint64_t)T, (uint64_t)(nu > 0 ? nu : 1)}, ud))
        return fail(LLPF_ERR_ARG, "simulate: the size of the outputs (n_filters * M * T * (nx + ny) * 8 bytes) or of U overflows");
    test_throw("simulate");
    CHK(use_device(b));
    {
        std::string err;
        if (simulate_prepare(model_id, err) != 0) return fail(LLPF_ERR_HIP, "simulate: " + err);
    }
    const bool upt = nu > 0 && u_per_traj;
    ChunkPipe pipe(b.stream);
    double *d_zero = nullptr, *d_state = nullptr;
    CHK(pipe.device(MAXU, d_zero));
    HIPC(hipMemsetAsync(d_zero, 0, sizeof(double) * MAXU, b.stream));
    CHK(pipe.device((size_t)FM * nx, d_state));
    // X, Y [F][T][M][n]; U [T][nu], or per trajectory [F][M][T][nu], packed [F][M][tc][nu]
    CHK(pipe.open(T, (size_t)(FM * w) * sizeof(double), {{X, (size_t)F, (size_t)M * nx}, {Y, (size_t)F, (size_t)M * ny}},
                  {{nu > 0 ? U : nullptr, upt ? (size_t)FM : 0, (size_t)nu, false}}));
    const int nt = pipe.chunk_bytes() > SIM_INFINITY_CACHE ? 1 : 0;
    for (int64_t c = 0; c < pipe.nchunk; ++c) {
        CHK(pipe.begin(c, c));
        const int64_t tc = pipe.tc;
        SimArgs a{};
        a.u = pipe.in(0);
        a.u_mstride = upt ? (int64_t)tc * nu : 0;
        a.u_fstride = upt ? (int64_t)M * tc * nu : 0;
        a.X = pipe.out(0);
        a.Y = pipe.out(1);
        a.xs = d_state; a.zero_u = d_zero;
        a.M = M; a.T = T; a.t0 = pipe.t0; a.Tc = (int32_t)tc; a.nu = nu; a.flags = flags; a.nt = nt; a.step0 = step0;
        a.t_index0 = t_index0; a.Ts = b.cfg.model.Ts;
        a.key0 = seed + b.key_off; a.key_stride = b.key_stride;      // filter f: seed + key_off + f * key_stride, as set_keys
        {
            ProfScope ps(b, LLPF_PROF_PROPAGATE);
            HIPC(launch_simulate(model_id, nx, ny, b.d_models, F, a, b.stream));
        }
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    HIPC(hipStreamSynchronize(b.stream));
    if (b.profiling) prof_collect(b);      // kernel time apart from the copies: LLPF_PROF_PROPAGATE of llpf_get_profile
    return LLPF_OK;
}
