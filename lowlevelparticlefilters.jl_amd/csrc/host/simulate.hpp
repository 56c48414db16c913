// host/simulate.hpp — simulate(pf, T, du) for M trajectories at once (llpf_simulate / llpf_bank_simulate; kernel: kernels/simulate.hpp).
// Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The steps are driven in chunks so that device memory stays bounded whatever T is: a chunk is Tc steps of every trajectory of every
// filter, Tc = min(T, 256, max(1, 64 MiB / bytes of one step's outputs)) — a chunk's outputs fit a 64 MiB staging buffer unless a single
// step is larger.  Chunk c runs into device staging buffer c % 2; a second stream copies it to pinned host buffer c % 2 while chunk c + 1
// runs, and the host moves it to the caller's arrays while chunk c + 2 runs.  The state x carries from chunk to chunk in a device buffer
// [F][nx][M], so a long run's prefix is a short run, bit for bit.  Outputs of a chunk beyond the Infinity Cache are stored nontemporal.
constexpr size_t SIM_CHUNK_BYTES = (size_t)64 << 20;
constexpr int64_t SIM_CHUNK_STEPS = 256;
constexpr size_t SIM_INFINITY_CACHE = (size_t)256 << 20;

// the copy stream, its events and the pinned staging of one simulation.  The destructor first waits for both streams (the copies in flight
// target these buffers and read the device buffers the caller declared before this object), then frees.
struct SimPipe {
    hipStream_t compute = nullptr;     // the bank's stream (not owned)
    hipStream_t copy = nullptr;
    hipEvent_t ev_k[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr}, ev_u[2] = {nullptr, nullptr};
    char* pinned[2] = {nullptr, nullptr};
    SimPipe() = default;
    SimPipe(const SimPipe&) = delete;
    SimPipe& operator=(const SimPipe&) = delete;
    ~SimPipe() {
        if (compute) hipStreamSynchronize(compute);
        if (copy) hipStreamSynchronize(copy);
        for (int i = 0; i < 2; ++i) {
            if (pinned[i]) hipHostFree(pinned[i]);
            for (hipEvent_t e : {ev_k[i], ev_c[i], ev_u[i]}) if (e) hipEventDestroy(e);
        }
        if (copy) hipStreamDestroy(copy);
    }
};

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
    const uint64_t w = (uint64_t)(X ? nx : 0) + (uint64_t)(Y ? ny : 0);
    uint64_t FM = 0, step_d = 0, total = 0, bytes = 0, ud = 0;
    if (__builtin_mul_overflow((uint64_t)F, (uint64_t)M, &FM) || __builtin_mul_overflow(FM, w, &step_d) ||
        __builtin_mul_overflow(step_d, (uint64_t)T, &total) || __builtin_mul_overflow(total, (uint64_t)sizeof(double), &bytes) ||
        __builtin_mul_overflow(FM, (uint64_t)T * (uint64_t)(nu > 0 ? nu : 1), &ud) || __builtin_mul_overflow(ud, (uint64_t)sizeof(double), &ud) ||
        bytes > (uint64_t)PTRDIFF_MAX || ud > (uint64_t)PTRDIFF_MAX)
        return fail(LLPF_ERR_ARG, "simulate: the size of the outputs (n_filters * M * T * (nx + ny) * 8 bytes) or of U overflows");
    test_throw("simulate");
    CHK(use_device(b));
    {
        std::string err;
        if (simulate_prepare(model_id, err) != 0) return fail(LLPF_ERR_HIP, "simulate: " + err);
    }
    const size_t step_bytes = (size_t)step_d * sizeof(double);
    const int64_t Tc = std::min<int64_t>(T, std::min<int64_t>(SIM_CHUNK_STEPS, std::max<int64_t>(1, (int64_t)(SIM_CHUNK_BYTES / step_bytes))));
    const int64_t nchunk = (T + Tc - 1) / Tc;
    const int nbuf = nchunk > 1 ? 2 : 1;
    const size_t chunk_d = (size_t)step_d * (size_t)Tc;
    const int nt = chunk_d * sizeof(double) > SIM_INFINITY_CACHE ? 1 : 0;
    const bool upt = nu > 0 && u_per_traj;
    const size_t chunk_u = nu > 0 ? (upt ? (size_t)FM * Tc * nu : (size_t)Tc * nu) : 0;
    // device buffers first: destroyed after the pipe has waited for the streams
    DevBuf<double> d_out[2], d_u[2], d_state, d_zero;
    CHK(d_zero.ensure(MAXU));
    HIPC(hipMemsetAsync(d_zero, 0, sizeof(double) * MAXU, b.stream));
    CHK(d_state.ensure((size_t)FM * nx));
    std::vector<double> upack[2];           // per-trajectory inputs of a chunk, packed [F][M][Tc][nu] for one contiguous copy
    SimPipe pipe;
    pipe.compute = b.stream;
    HIPC(hipStreamCreateWithFlags(&pipe.copy, hipStreamNonBlocking));
    for (int i = 0; i < nbuf; ++i) {
        CHK(d_out[i].ensure(chunk_d));
        if (nu > 0) CHK(d_u[i].ensure(chunk_u));
        if (upt) upack[i].resize(chunk_u);
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&pipe.pinned[i]), chunk_d * sizeof(double), hipHostMallocDefault));
        HIPC(hipEventCreateWithFlags(&pipe.ev_k[i], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&pipe.ev_c[i], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&pipe.ev_u[i], hipEventDisableTiming));
    }
    // chunk c's outputs from pinned buffer c % 2 into the caller's [F][T][M][n] arrays (one contiguous range per filter and output)
    auto drain = [&](int64_t c) -> int {
        const int s = (int)(c & 1);
        const int64_t t0 = c * Tc, tc = std::min<int64_t>(Tc, T - t0);
        HIPC(hipEventSynchronize(pipe.ev_c[s]));
        const double* src = reinterpret_cast<const double*>(pipe.pinned[s]);
        if (X) {
            const size_t n = (size_t)tc * M * nx;
            for (int f = 0; f < F; ++f) memcpy(X + ((size_t)f * T + t0) * M * nx, src + (size_t)f * n, n * sizeof(double));
            src += (size_t)F * n;
        }
        if (Y) {
            const size_t n = (size_t)tc * M * ny;
            for (int f = 0; f < F; ++f) memcpy(Y + ((size_t)f * T + t0) * M * ny, src + (size_t)f * n, n * sizeof(double));
        }
        return LLPF_OK;
    };
    for (int64_t c = 0; c < nchunk; ++c) {
        const int s = (int)(c & 1);
        const int64_t t0 = c * Tc, tc = std::min<int64_t>(Tc, T - t0);
        if (c >= 2) HIPC(hipStreamWaitEvent(b.stream, pipe.ev_c[s], 0));     // staging s has been copied out (chunk c - 2)
        if (nu > 0) {
            if (upt) {
                if (c >= 2) HIPC(hipEventSynchronize(pipe.ev_u[s]));              // the copy of chunk c - 2 has read upack[s]
                double* dst = upack[s].data();
                for (uint64_t r = 0; r < FM; ++r, dst += (size_t)tc * nu) memcpy(dst, U + ((size_t)r * T + t0) * nu, sizeof(double) * tc * nu);
                HIPC(hipMemcpyAsync(d_u[s], upack[s].data(), sizeof(double) * FM * tc * nu, hipMemcpyHostToDevice, b.stream));
                HIPC(hipEventRecord(pipe.ev_u[s], b.stream));
            } else {
                HIPC(hipMemcpyAsync(d_u[s], U + (size_t)t0 * nu, sizeof(double) * tc * nu, hipMemcpyHostToDevice, b.stream));
            }
        }
        SimArgs a{};
        a.u = nu > 0 ? d_u[s].p : nullptr;
        a.u_mstride = upt ? (int64_t)tc * nu : 0;
        a.u_fstride = upt ? (int64_t)M * tc * nu : 0;
        a.X = X ? d_out[s].p : nullptr;
        a.Y = Y ? d_out[s].p + (X ? (size_t)FM * tc * nx : 0) : nullptr;
        a.xs = d_state; a.zero_u = d_zero;
        a.M = M; a.T = T; a.t0 = t0; a.Tc = (int32_t)tc; a.nu = nu; a.flags = flags; a.nt = nt; a.step0 = step0;
        a.t_index0 = t_index0; a.Ts = b.cfg.model.Ts;
        a.key0 = seed + b.key_off; a.key_stride = b.key_stride;      // filter f: seed + key_off + f * key_stride, as set_keys
        {
            ProfScope ps(b, LLPF_PROF_PROPAGATE);
            HIPC(launch_simulate(model_id, nx, ny, b.d_models, F, a, b.stream));
        }
        HIPC(hipEventRecord(pipe.ev_k[s], b.stream));
        HIPC(hipStreamWaitEvent(pipe.copy, pipe.ev_k[s], 0));
        HIPC(hipMemcpyAsync(pipe.pinned[s], d_out[s], (size_t)step_d * tc * sizeof(double), hipMemcpyDeviceToHost, pipe.copy));
        HIPC(hipEventRecord(pipe.ev_c[s], pipe.copy));
        if (c >= 1) CHK(drain(c - 1));
    }
    CHK(drain(nchunk - 1));
    HIPC(hipStreamSynchronize(b.stream));
    if (b.profiling) prof_collect(b);      // kernel time apart from the copies: LLPF_PROF_PROPAGATE of llpf_get_profile
    return LLPF_OK;
}
