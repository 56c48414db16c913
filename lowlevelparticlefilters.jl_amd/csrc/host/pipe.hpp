// host/pipe.hpp — the chunked staging pipeline of the batch verbs.  Part of capi.hip (one translation unit).  Its callers: bank_simulate
// (host/simulate.hpp: llpf_simulate, llpf_bank_simulate), and kf_forward and kf_smooth (host/kfbank.hpp: the run and the smooth of the
// Kalman banks, host/kalman.hpp, and of the unscented banks, host/ukf.hpp).
// ------------------------------------------------------------------------------------------------
// The T steps of a call are driven in chunks so that device and pinned memory stay bounded whatever T is: a chunk is
// Tc = min(T, 256, max(1, 64 MiB / bytes the caller counts per step)) steps.  Launch i runs its chunk into device staging buffer i % 2; a
// second stream copies it to pinned host buffer i % 2 while launch i + 1 runs, and the host moves it into the caller's arrays while launch
// i + 2 runs.  The inputs of a chunk go the other way on the compute stream in front of the launch: a shared input as a slice of the
// caller's array, a per-row input packed on the host for one contiguous copy.  ChunkPipe owns all of it (streams, events, pinned and
// device buffers, packs) and the order of the waits; a caller describes its arrays, fills its kernel's arguments and launches.
constexpr size_t CHUNK_BYTES = (size_t)64 << 20;
constexpr int64_t CHUNK_STEPS = 256;

// n = the product of the factors, a number of doubles: false when it, or its size in bytes, does not fit ptrdiff_t
static bool doubles_fit(std::initializer_list<uint64_t> factors, uint64_t& n) {
    n = 1;
    for (uint64_t f : factors)
        if (__builtin_mul_overflow(n, f, &n)) return false;
    return n <= (uint64_t)PTRDIFF_MAX / sizeof(double);
}

// one output: the caller's array dst [rows][T][w] (null: not asked for, nothing is staged).  The staging of a chunk of tc steps holds
// [rows][tc][w] of every output that has a dst, in list order.
struct ChunkOut { double* dst; size_t rows, w; };
// one input (src null: the model has none): [T][n] shared by all rows (rows = 0), or [rows][T][n], which reaches the device packed as
// [rows][tc][n], or as [tc][rows][n] where the kernel reads it time-major
struct ChunkIn { const double* src; size_t rows, n; bool time_major; };

struct ChunkPipe {
    int64_t Tc = 0, nchunk = 0;
    int64_t t0 = 0, tc = 0;             // the chunk of the launch begun last: steps [t0, t0 + tc)

    explicit ChunkPipe(hipStream_t compute_) : compute(compute_) {}
    ChunkPipe(const ChunkPipe&) = delete;
    ChunkPipe& operator=(const ChunkPipe&) = delete;
    // waits for both streams first: the copies and launches in flight use the buffers released here and, after this body, by the members
    ~ChunkPipe() {
        hipStreamSynchronize(compute);
        if (copy) hipStreamSynchronize(copy);
        for (Slot& s : slot) {
            if (s.pinned) hipHostFree(s.pinned);
            for (hipEvent_t e : {s.ev_k, s.ev_c, s.ev_u}) if (e) hipEventDestroy(e);
        }
        if (copy) hipStreamDestroy(copy);
    }

    // the one chunk rule.  step_bytes: what the caller counts against the staging limit (0: nothing per step scales with the bank)
    static int64_t chunk_steps(int64_t T, size_t step_bytes) {
        return std::min<int64_t>(T, std::min<int64_t>(CHUNK_STEPS, step_bytes ? std::max<int64_t>(1, (int64_t)(CHUNK_BYTES / step_bytes)) : CHUNK_STEPS));
    }
    // a device buffer of n doubles that a launch of this pipeline reads or writes (a carried state): released with the staging
    int device(size_t n, double*& p) {
        held.emplace_back();
        CHK(held.back().ensure(n));
        p = held.back();
        return LLPF_OK;
    }
    // allocates everything the T steps need; no launch has run when this fails
    int open(int64_t T_, size_t step_bytes, std::vector<ChunkOut> outs_, std::vector<ChunkIn> ins_) {
        T = T_; outs = std::move(outs_); ins = std::move(ins_);
        for (const ChunkOut& o : outs) if (o.dst) step_d += o.rows * o.w;
        for (const ChunkIn& in : ins) if (in.src && in.rows) packs = true;
        Tc = chunk_steps(T, step_bytes);
        nchunk = (T + Tc - 1) / Tc;
        HIPC(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
        for (int i = 0; i < (nchunk > 1 ? 2 : 1); ++i) {
            Slot& s = slot[i];
            if (step_d) {           // (nothing staged per step: no pinned memory, no copy)
                CHK(s.d_out.ensure(step_d * Tc));
                HIPC(hipHostMalloc(reinterpret_cast<void**>(&s.pinned), chunk_bytes(), hipHostMallocDefault));
            }
            s.d_in.resize(ins.size());
            s.pack.resize(ins.size());
            for (size_t k = 0; k < ins.size(); ++k) {
                if (!ins[k].src) continue;
                const size_t n = (ins[k].rows ? ins[k].rows : 1) * (size_t)Tc * ins[k].n;
                CHK(s.d_in[k].ensure(n));
                if (ins[k].rows) s.pack[k].resize(n);
            }
            HIPC(hipEventCreateWithFlags(&s.ev_k, hipEventDisableTiming));
            HIPC(hipEventCreateWithFlags(&s.ev_c, hipEventDisableTiming));
            HIPC(hipEventCreateWithFlags(&s.ev_u, hipEventDisableTiming));
        }
        return LLPF_OK;
    }
    size_t chunk_bytes() const { return step_d * (size_t)Tc * sizeof(double); }      // the staging of a full chunk

    // launch i runs chunk c (a backward pass walks the chunks in reverse): waits until slot i % 2 can be used again, then stages the inputs
    int begin(int64_t i, int64_t c) {
        Slot& s = slot[i & 1];
        cur = i;
        s.t0 = t0 = c * Tc;
        s.tc = tc = std::min<int64_t>(Tc, T - t0);
        if (i >= 2 && step_d) HIPC(hipStreamWaitEvent(compute, s.ev_c, 0));      // the staging has been copied out (launch i - 2)
        if (i >= 2 && packs) HIPC(hipEventSynchronize(s.ev_u));                  // the copies of launch i - 2 have read the packs
        for (size_t k = 0; k < ins.size(); ++k) {
            const ChunkIn& in = ins[k];
            if (!in.src) continue;
            const double* h = in.src + (size_t)t0 * in.n;
            if (in.rows) {
                double* p = s.pack[k].data();
                if (in.time_major) {
                    for (int64_t j = 0; j < tc; ++j)
                        for (size_t r = 0; r < in.rows; ++r)
                            memcpy(p + ((size_t)j * in.rows + r) * in.n, h + (r * (size_t)T + j) * in.n, sizeof(double) * in.n);
                } else {
                    for (size_t r = 0; r < in.rows; ++r) memcpy(p + r * (size_t)tc * in.n, h + r * (size_t)T * in.n, sizeof(double) * tc * in.n);
                }
                h = p;
            }
            HIPC(hipMemcpyAsync(s.d_in[k], h, sizeof(double) * (in.rows ? in.rows : 1) * tc * in.n, hipMemcpyHostToDevice, compute));
        }
        if (packs) HIPC(hipEventRecord(s.ev_u, compute));
        return LLPF_OK;
    }
    // where the launch begun last reads input k and writes output k (positions in the lists given to open; null as src / dst is)
    const double* in(size_t k) const { return ins[k].src ? slot[cur & 1].d_in[k].p : nullptr; }
    double* out(size_t k) const {
        if (!outs[k].dst) return nullptr;
        double* o = slot[cur & 1].d_out.p;
        for (size_t j = 0; j < k; ++j) if (outs[j].dst) o += outs[j].rows * (size_t)tc * outs[j].w;
        return o;
    }
    // after the launch: its staging to the pinned buffer on the copy stream, and the launch before it into the caller's arrays
    int end() {
        if (!step_d) return LLPF_OK;
        Slot& s = slot[cur & 1];
        HIPC(hipEventRecord(s.ev_k, compute));
        HIPC(hipStreamWaitEvent(copy, s.ev_k, 0));
        HIPC(hipMemcpyAsync(s.pinned, s.d_out, step_d * (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, copy));
        HIPC(hipEventRecord(s.ev_c, copy));
        return cur >= 1 ? drain(slot[(cur - 1) & 1]) : LLPF_OK;
    }
    // the last launch into the caller's arrays
    int finish() { return step_d ? drain(slot[cur & 1]) : LLPF_OK; }

private:
    struct Slot {
        DevBuf<double> d_out;                       // the outputs of a chunk, as ChunkOut says
        std::vector<DevBuf<double>> d_in;           // input k of a chunk
        std::vector<std::vector<double>> pack;      // ... and its host pack where it is per row
        char* pinned = nullptr;
        hipEvent_t ev_k = nullptr, ev_c = nullptr, ev_u = nullptr;      // the launch is done, its copy out is done, its inputs are in
        int64_t t0 = 0, tc = 0;                     // the chunk that sits in this slot
    };
    // the chunk in slot s from its pinned buffer into the caller's arrays: one contiguous range per output and row
    int drain(Slot& s) {
        HIPC(hipEventSynchronize(s.ev_c));
        const double* src = reinterpret_cast<const double*>(s.pinned);
        for (const ChunkOut& o : outs) {
            if (!o.dst) continue;
            const size_t n = (size_t)s.tc * o.w;
            for (size_t r = 0; r < o.rows; ++r, src += n) memcpy(o.dst + (r * (size_t)T + (size_t)s.t0) * o.w, src, n * sizeof(double));
        }
        return LLPF_OK;
    }

    hipStream_t compute, copy = nullptr;      // the bank's stream (not owned) and the copy stream
    Slot slot[2];
    std::vector<DevBuf<double>> held;
    std::vector<ChunkOut> outs;
    std::vector<ChunkIn> ins;
    size_t step_d = 0;                        // doubles staged out per step
    bool packs = false;                       // some input is packed on the host: ev_u guards the reuse of a pack
    int64_t T = 0, cur = 0;
};
