// kernels/resprop.hpp — k_resprop, the fused predict!.  Part of kernels.hip (one translation unit, namespace llpf).
// ------------------------------------------------------------------------------------------------
// k_resprop — the fused predict!: finalize + shouldresample + resample + propagate [+ weight of the next
// correct!] in ONE launch.  A block owns a tile of 1024 SOURCE particles; it derives which outputs its sources
// produce ([c_start, c_end), from the ancestor counts) and propagates exactly those outputs, reading its
// sources' states (an 8 KB window per dimension: L1/L2 hits) and writing x, w (and j, kept for the accessor and
// for the reference's "stale j" corner) coalesced.  No ancestor array round trip, no separate propagate launch.
// Load balance: a tile produces ~1024 outputs +- a few % for i.i.d.-like weights; a tile holding very heavy
// particles loops over more 256-output chunks (worst case ESS -> 1: one block does everything; still far faster
// than the serial reference).
// The per-output arithmetic is the same sequence as k_step's, so fused and unfused paths are bit-identical.
// ------------------------------------------------------------------------------------------------
template <class T> DEV T ld_off(const T* base, uint32_t byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
template <class T> DEV void st_off(T* base, uint32_t byte_off, T v) {
    *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// stores of the output loop are write-through (wt_store in reduce.hpp says why)
#ifndef LLPF_RBX_TAB
#define LLPF_RBX_TAB 1      /* RBLin with a compile-time split: generator tables in LDS + owner table, like the plain model's kernel */
#endif
#ifndef LLPF_RBX_W4
#define LLPF_RBX_W4 1       /* ... and four waves per SIMD */
#endif
#ifndef LLPF_RBX_WT
#define LLPF_RBX_WT 1       /* ... and write-through stores (same box, us per timestep at N = 1e6: run-time split 30.0; compile-time split 24.6; + tables 23.1; + four waves 23.3; + these 22.7 — profiles/r06_rbpf_lean_ab.txt) */
#endif
#ifndef LLPF_RESPROP_PF
#define LLPF_RESPROP_PF 2      /* rounds of the split-schedule output loop whose sources are requested together (1.6e7 particles, plain stores: 1: 240.5, 2: 236, 4: 250 us) */
#endif
// the fixed part of a level-3 launch (k_resprop<..., LEVEL >= 3>; EXPERIMENTS: the fixed part around the loop), each step switchable for A/B builds
#ifndef LLPF_LEAN_TAIL
#define LLPF_LEAN_TAIL 1       /* the tail in one barrier: block_flush instead of block_max + __syncthreads_or + acc_max + WeightAcc::flush */
#endif
#ifndef LLPF_LEAN_HEAD
#define LLPF_LEAN_HEAD 1       /* head and scan with the argument values of such a launch compiled in, 1 / M from the host (res_head / res_counts<..., LEAN>) */
#endif
// wave priority by progress in the rounds of the level-3 output loop (shared/llpf_loop_prio.h has the maps; EXPERIMENTS: the output
// loop's waves side by side)
#ifndef LLPF_LOOP_PRIO
#define LLPF_LOOP_PRIO 1       /* 0: one priority for the whole loop, waves served by age; 1: map A, min(2, rounds left - 1); 2: map B, min(3, rounds left - 1) */
#endif
#include "../shared/llpf_loop_prio.h"
// a round of the level-3 output loop without its repeated work (EXPERIMENTS: a round without its repeated work): LLPF_LEAN_ROUND=0 is the loop
// as it was; LLPF_LEAN_ROUND_ITEMS picks single items for A/B builds.  None changes a bit of any result.
#ifndef LLPF_LEAN_ROUND
#define LLPF_LEAN_ROUND 1
#endif
#define LLPF_LR_QFIX   1       /* the quantum is the fixed-point exp-weight shifted (llpf_q64_from_fix96_k33), not formed a second time from e */
#define LLPF_LR_NANFLAG 2      /* NaN exp-weights: a lane flag instead of WeightAcc's 64-bit count (only its being non-zero is ever used); not in the default: alone it measured no gain (EXPERIMENTS) */
#define LLPF_LR_BZ     4       /* B u by one add (LinGauss::dynamics_bz), not two adds and a select on the uniform has_u */
#define LLPF_LR_NOPAD  8       /* no padding test: every output of such a launch is below M == N (launch_resprop_t refuses any other) */
#define LLPF_LR_POW2   16      /* the uniforms' power-of-two scalings folded (llpf_normals_tab_s) */
#define LLPF_LR_CARRY  32      /* the 128-bit running sum as one carry chain (unsigned __int128) */
#ifndef LLPF_LEAN_ROUND_ITEMS
#define LLPF_LEAN_ROUND_ITEMS (LLPF_LR_QFIX | LLPF_LR_BZ | LLPF_LR_NOPAD | LLPF_LR_POW2)
#endif
#define LLPF_LR_BITS (LLPF_LEAN_ROUND ? (LLPF_LEAN_ROUND_ITEMS) : 0)
#define LLPF_LR_NOMAX  64      /* no NaN flag of the weights in the round (k_resprop<..., LEVEL = 4>: the launch leaves no running maximum); not one of LLPF_LEAN_ROUND's items, set by the level alone */
// a level-3 launch that another one follows leaves no running maximum behind (LEVEL = 4; EXPERIMENTS: the tail's accumulators): LLPF_SKIP_MAX=0
// compiles neither the kernel nor the plan's use of it (host/run_plan.hpp), and every launch is the code as it was
#ifndef LLPF_SKIP_MAX
#define LLPF_SKIP_MAX 1
#endif
#define LLPF_RB_PLAIN_ST (Model::RB && !(model_lean<Model>::value && LLPF_RBX_WT))
// store policy of the output loop (Mem<>::st): 1 = write-through (sc1), 0 = plain, 2 = nontemporal
#ifndef LLPF_RESPROP_ST
#define LLPF_RESPROP_ST 1
#endif
// ... and of the steps that do not resample (every output reads its own index: nothing a store leaves in the L2 is read again by this launch)
#ifndef LLPF_RESPROP_ST_ID
#define LLPF_RESPROP_ST_ID LLPF_RESPROP_ST
#endif
#ifndef LLPF_RESPROP_ID2
#define LLPF_RESPROP_ID2 1     /* steps that do not resample, split-schedule form: two adjacent outputs per thread, 16-byte accesses (LLPF_OUTPUT_LOOP_ID2) */
#endif
#ifndef LLPF_RESPROP_LD_ID
#define LLPF_RESPROP_LD_ID 0      /* 1: the sources of such a step are read nontemporal as well */
#endif
#define LLPF_STCOH ((LLPF_WT && !LLPF_RB_PLAIN_ST) ? STP : COH)
#define LLPF_STCOH0 ((LLPF_WT && !LLPF_RB_PLAIN_ST) ? LLPF_RESPROP_ST : 0)
// STW = false: the weights formed here are not stored (k_resprop<..., LEVEL >= 1>: nobody reads them)
// LR: the LLPF_LR_* items of the level-3 round (0 everywhere else)
template <class Model, int NX, int NY, bool WEIGHT, bool COH = false, bool LTAB = false, bool STW = true, int LR = 0>
struct PropCtx {
    const BankDev& b;
    const Model& model;
    const ModelD* md;
    const StepArgs& st;
    const double* y;
    const double* __restrict__ xc;
    double* __restrict__ xn;
    double* w;             // weights in front of this launch (read: w_prev of a step that does not resample)
    double* wn;            // weights this launch forms (BankDev::w_next)
    uint32_t k0, k1;
    uint32_t pstep;        // Philox step of this predict! (step_base + st.step)
    int ablate;
    double off;            // bound of the new weights (offset of their exp-sums)
    uint64_t* qnext;       // quanta of the new weights
    const double* rng_lg = nullptr;   // the block's copy of the generator's tables in LDS , or nullptr: the
    const double* rng_sc = nullptr;   //   tables in constant memory (a global load through the GOT per lookup)
    const double* bz = nullptr;       // LLPF_LR_BZ: the model's input term (LinGauss::input_term)
    // propagate output o from source src with previous log-weight wprev; returns the new log-weight
    // Addresses are a uniform plane base (SGPRs) + a 32-bit byte offset (one VGPR): Ns * 8 < 2^32 is checked at create.
    // the source's state (nontemporal: C2 22.8 against 20.7 us — duplicated ancestors are re-read from the L2)
    template <bool NTL = false>
    DEV void fetch(uint32_t src, double* xp) const {
        const int64_t Ns = b.Ns;
        const uint32_t so = src << 3;
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            if constexpr (NTL) xp[d] = __builtin_nontemporal_load(reinterpret_cast<const double*>(reinterpret_cast<const char*>(xc + (size_t)d * Ns) + so));
            else xp[d] = Mem<COH>::ld_off(xc + (size_t)d * Ns, so);
        }
    }
    template <int STP = LLPF_RESPROP_ST, bool NTL = false>
    DEV double one(uint32_t src, uint32_t o, double wprev, bool& bad, double* xs) const {
        double xp[NX];
        fetch<NTL>(src, xp);
        return one_x<STP>(xp, o, wprev, bad, xs);
    }
    // ... from the state xp of its source (fetch); STP: the store policy of this call (LLPF_RESPROP_ST / LLPF_RESPROP_ST_ID), or -1: nothing is
    // stored here — the caller stores xs and the returned weight itself (LLPF_OUTPUT_LOOP_ID2: two outputs per 16-byte store)
    template <int STP = LLPF_RESPROP_ST>
    DEV double one_x(const double* xp, uint32_t o, double wprev, bool& bad, double* xs) const {
        const int64_t Ns = b.Ns;
        const uint32_t oo = o << 3;
        double fx[NX], xi[NX], nz[NX];
        if constexpr (Model::RB) {     // Rao-Blackwellized model: own noise structure, and correct! updates xl before the store
            if constexpr (LTAB) model.rb_propagate(xp, o, pstep, k0, k1, st.rb_pred + blockIdx.y, xs, rng_lg, rng_sc);
            else model.rb_propagate(xp, o, pstep, k0, k1, st.rb_pred + blockIdx.y, xs);
            double wr = wprev;
            if (WEIGHT) {
                if (st.has_y) wr = wr + model.rb_weight(xs, y, st.rb_corr + blockIdx.y, o == 0);
                if (o >= (uint32_t)b.N) wr = -LLPF_INF;
                bad = bad || (wr != wr);
                if constexpr (STP >= 0) Mem<LLPF_STCOH>::st_off(wn, oo, wr);
            }
            if constexpr (STP >= 0) {
#pragma unroll
                for (int d = 0; d < NX; ++d) Mem<LLPF_STCOH>::st_off(xn + (size_t)d * Ns, oo, xs[d]);
            }
            return wr;
        }
#ifdef LLPF_DEVTOOLS   /* ablation switches for performance experiments (results invalid); not in production builds */
        if (!(ablate & 4)) { if constexpr ((LR & LLPF_LR_BZ) != 0) model.dynamics_bz(xp, bz, fx); else model.dynamics(xp, fx); }
        else { for (int d = 0; d < NX; ++d) fx[d] = xp[d]; }
        if (!(ablate & 1)) {
            if constexpr (LTAB && (LR & LLPF_LR_POW2) != 0) llpf_normals_tab_s(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, rng_lg, rng_sc);
            else if constexpr (LTAB) llpf_normals_tab(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, rng_lg, rng_sc);
            else llpf_normals(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi);
        }
        else { for (int d = 0; d < NX; ++d) xi[d] = 0.25 * (double)(o & 7); }
#else
        if constexpr ((LR & LLPF_LR_BZ) != 0) model.dynamics_bz(xp, bz, fx);
        else model.dynamics(xp, fx);
        if constexpr (LTAB && (LR & LLPF_LR_POW2) != 0) llpf_normals_tab_s(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, rng_lg, rng_sc);
        else if constexpr (LTAB) llpf_normals_tab(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi, rng_lg, rng_sc);
        else llpf_normals(o, pstep, LLPF_STREAM_DYNAMICS, k0, k1, NX, xi);
#endif
        gauss_sample_c<NX>((gauss_cptr)&md->df, xi, nz);
#pragma unroll
        for (int d = 0; d < NX; ++d) {
            xs[d] = fx[d] + nz[d];
            if constexpr (STP >= 0) Mem<LLPF_STCOH>::st_off(xn + (size_t)d * Ns, oo, xs[d]);
        }
        double wv = wprev;
        if (WEIGHT) {
#ifdef LLPF_DEVTOOLS
            if (st.has_y && !(ablate & 4)) {
#else
            if (st.has_y) {
#endif
                double g[NY], v[NY];
                model.measurement(xs, g);
#pragma unroll
                for (int k = 0; k < NY; ++k) v[k] = y[k] - g[k];
                wv = wv + gauss_logpdf_c<NY>((gauss_cptr)&md->dg, v);
            }
            if constexpr (!(LR & LLPF_LR_NOPAD)) { if (o >= (uint32_t)b.N) wv = -LLPF_INF; }
            if constexpr (!(LR & LLPF_LR_NOMAX)) bad = bad || (wv != wv);
#ifdef LLPF_DEVTOOLS
            if (!(ablate & 8))
#endif
            if constexpr (STP >= 0 && STW) Mem<LLPF_STCOH>::st_off(wn, oo, wv);
        }
        return wv;
    }
};

// WeightAcc::add of the level-3 round (need_e2 false, e not wanted): the same sum S and the same quantum, by the LLPF_LR_* items of LR.
// `nan` stands for WeightAcc::bad under LLPF_LR_NANFLAG; the kernel hands block_flush bad = nan ? 1 : 0, so the ballot it takes is the same.
template <int LR>
DEV uint64_t lean_acc_add(WeightAcc& wa, bool& nan, double w, double off, int K) {
    const double e = llpf_exp_le0(w - off);
    if constexpr ((LR & LLPF_LR_NANFLAG) != 0) nan = nan || (e != e);
    else wa.bad += (e != e) ? 1u : 0u;
    const llpf_u128 fx = llpf_fix96_unit(e);
    if constexpr ((LR & LLPF_LR_CARRY) != 0) {
        const unsigned __int128 t = (((unsigned __int128)wa.S.hi << 64) | wa.S.lo) + (((unsigned __int128)fx.hi << 64) | fx.lo);
        wa.S.lo = (uint64_t)t; wa.S.hi = (uint64_t)(t >> 64);
    } else wa.S = llpf_u128_add(wa.S, fx);
    if constexpr ((LR & LLPF_LR_QFIX) != 0) return llpf_q64_from_fix96_k33(fx, K);
    else return llpf_q64_unit(e, K);
}

#ifdef LLPF_DEVTOOLS
// (not a constant: equal quanta would give every tile exactly 1024 outputs and no wave a fifth round — the high word of the fixed-point
// value, one shift, keeps the ancestor counts near the real ones)
DEV uint64_t ablated_acc_add(WeightAcc& wa, double w, double off, int K) {
    const llpf_u128 fx = llpf_fix96_unit(llpf_exp_le0(w - off));
    wa.S = llpf_u128_add(wa.S, fx);
    return fx.hi << (K - 32);
}
#endif

// per-thread running sum of quanta keyed by destination tile; flushed to LDS (first 8 tiles of the block's output
// range) or straight to the global tile sums (heavier blocks) whenever the tile changes
struct TileSum {
    int32_t tcur;
    uint64_t run;
    DEV void init() { tcur = -1; run = 0; }
    DEV void flush(uint64_t* sh_tq, uint64_t* tq_global, int32_t tbase) {
        if (run) {
            const int32_t idx = tcur - tbase;
            // two atomics the compiler cannot merge into ONE on a generic pointer (different scopes): behind a flat atomic it can no longer
            // tell LDS from memory traffic, and every wait of the output loop after it — all of them, round the back edge — becomes a full
            // drain of both counters (the gather's consumption: vmcnt(0) where nothing but the gather's own second half need be waited for)
            if (idx >= 0 && idx < 8) __hip_atomic_fetch_add(sh_tq + idx, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_fetch_add(tq_global + tcur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        run = 0;
    }
    DEV void add(uint32_t o, uint64_t q, uint64_t* sh_tq, uint64_t* tq_global, int32_t tbase) {
        const int32_t t = (int32_t)(o >> 10);
        if (t != tcur) { flush(sh_tq, tq_global, tbase); tcur = t; }
        run += q;
    }
};
static_assert(TILE == 1024, "TileSum assumes 1024-particle tiles");

// leading scalar kernel arguments: preloaded into SGPRs by the command processor (-mllvm -amdgpu-kernarg-preload-count;
// a struct passed by value as the FIRST argument disables the preload, which is why these are not left inside BankDev)
#define LLPF_HOT_PARAMS uint64_t* hot_acc, uint64_t* hot_tileq, FilterScal* hot_scal, uint32_t* hot_flag, const uint64_t* hot_quanta, \
                        int hot_F, int hot_P2, int hot_parity
#define LLPF_HOT_ARGS(b, a) (b).acc, (b).tileq, (b).scal, (b).bank_flag, (b).quanta, (b).F, (b).P2, (a).parity

// ONE: the filter is a single tile (launched only when P2 == 1): a failed bound test is redone inside this kernel
// LEVEL: what the launch leaves out, a RunLevel (host/run_plan.hpp: planned by make_run_plan, per launch by launch_level).  Each level is
// the one below it and one thing more; SKIPW, SKIPA and LEAN below are LEVEL >= 1, >= 2 and >= 3.
// SKIPW: a run at resample_threshold 1 (every step resamples, so the prior of every weight is log(1/N) and the next head
// consumes only the integer sums and the quanta): the weights formed here are not stored — 8 of the 44 bytes an output writes, one of its
// five stores.  The only reader of those weights, the exact redo of a failed bound test, has the host form them again first, from the
// states in memory.  A head that would not resample (no quanta at all) asks for that redo instead of reading the weights.
// SKIPA (never a run's last launch, which is WEIGHT = false): the rounds with an owner store no ancestor either — 4 of
// the remaining 36 bytes, one of the four stores.  The next launch of the run overwrites all of them unread, with one exception: its
// rounds of [c_end, M) read the previous ancestor of their own output, and only output M - 1 can be such an output (its threshold is the
// only one that can reach bins[N]: tests/test_stale_corner.py).  That entry is kept current: stored once behind the loop by the block
// that owns output M - 1, and by the rounds of [c_end, M) as ever.
// What SKIPW says about the run is compiled in: past the head every launch resamples (threshold 1: decide_resample returns 1, and a head
// whose quanta sum to zero has asked for the redo, NO_TOT0), so there is no arm for a step that does not — it could not run anyway, the
// weights it would read were never stored — and no sum of squares (host/fallback.hpp: need_e2 is 0 at threshold 1).
// LEAN: the run also resamples systematically and wants no weighted means — only
// res_counts<LLPF_RESAMPLE_SYSTEMATIC> is instantiated, and there is no xm[], no block_store_xm and no test of either.  The same
// arithmetic, counters, stores and visiting order: the form only drops tests and arms that such a run never takes.
// Its head and scan hold the argument values of such a launch as constants (res_head / res_counts<..., LEAN>; launch_resprop_t refuses a
// level-3 launch with others), and its tail is block_flush's one barrier: all blocks of a 10^6-particle filter are resident together and
// pass head, scan and tail in lockstep, so nothing hides a barrier or an argument test there.
// NOMAX (LEVEL = 4, a launch's level only: the plan's stays 3, and launch_level gives 4 to the level-3 launches that another launch with
// a weighting phase follows): the launch leaves no running maximum of its weights and reads none.  The head behind it is a level-3 or
// level-4 head, whose offset is the bound and whose bound test reads the integer sums and the NaN count; the maximum such a head combines
// goes only into FilterScal::mtrue and ::wmax, which the head after it overwrites unread (DESIGN.md §4 lists every reader).  So the rounds
// keep no bmax and no NaN flag of the weights, the tail is block_flush_sums (no wave_max, no atomicMax), and the launch's own head requests
// no ACC_PM line and publishes NaN in both fields (res_head<..., NOMAX>).  The run's last weighting launch stays level 3: the head behind
// it is the general one of the run's last launch, and what that head publishes is what the run leaves.
template <class Model, int NX, int NY, bool WEIGHT, bool ACC, bool AUX = false, bool ONE = false, int LEVEL = 0>
// amdgpu_waves_per_eu(4): the ~3.8 blocks per CU of a 10^6-particle filter must be resident together (<= 128 VGPRs); the
// larger state dimensions would spill under that cap and keep the compiler's choice; the Rao-Blackwellized propagate uses
// 130-156 VGPRs and is pinned to three waves per SIMD (<= 168): twice in this round an unrelated change pushed it past 170 and
// cost it 28 %
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(((!Model::RB || (model_lean<Model>::value && LLPF_RBX_W4)) && NX <= 2 && NY <= 2 && !ONE) ? 4 : (Model::RB ? 3 : 1)))) void k_resprop(LLPF_HOT_PARAMS, BankDev b_in, const ModelD* __restrict__ models, ResArgs a_in, StepArgs st) {
    constexpr bool SKIPW = LEVEL >= 1, SKIPA = LEVEL >= 2, LEAN = LEVEL >= 3, NOMAX = LEVEL >= 4;
    static_assert(!NOMAX || (LLPF_SKIP_MAX && LLPF_LEAN_TAIL && LLPF_LEAN_HEAD), "level 4 is level 3's head and tail without the maximum");
    // what the head's first loads are addressed with arrives in SGPRs with the wave (kernarg preload) instead of through a
    // scalar load of the argument block: one memory round trip less at the start of every launch
    BankDev b = b_in;
    b.acc = hot_acc; b.tileq = hot_tileq; b.scal = hot_scal; b.bank_flag = hot_flag; b.quanta = const_cast<uint64_t*>(hot_quanta);
    b.F = hot_F; b.P2 = hot_P2;
    ResArgs a = a_in;
    a.parity = hot_parity;
    a.mode = RES_FINALIZE | RES_RESAMPLE;        // what launch_resprop always passes: known here, the head's first loads then wait for no scalar load of the argument block
    __shared__ ResShared sh;
    __shared__ double sm_max[BLOCK / 64];
    __shared__ uint64_t sm_acc[BLOCK / 64][5];
    __shared__ uint64_t sh_tq[8];
    __shared__ uint64_t sm_fl[BLOCK / 64][8];      // block_flush (level 3; the levels below use sm_max and sm_acc)
    __shared__ double sm_x[BLOCK / 64][MAXD];
    constexpr bool RBFAT = Model::RB && !(model_lean<Model>::value && LLPF_RBX_TAB);      // run-time split: no registers to spare for the tables (occupancy 3 -> 2)
    constexpr bool OWN_TABLE = !RBFAT;
    __shared__ __attribute__((aligned(16))) uint32_t sh_own[OWN_TABLE ? OWN_CAP : 4];
    __shared__ __attribute__((aligned(16))) double sh_rng_lg[2 * LLPF_RNG_LG_ENTRIES], sh_rng_sc[2 * LLPF_RNG_SC_ENTRIES];
    // Wave priority by phase: the head / counts / tail phases are short and latency-bound (loads, LDS, barriers, atomics), the
    // output loop is long and issue-bound.  The waves of a CU's four blocks are otherwise served oldest first, so the
    // youngest block's head is starved by the older blocks' loops and the SIMD ends the launch with that block's loop alone
    // (in-kernel stamps, tools/dbg/timing_report.py).  Same-box A/B: C2 27.0 -> 26.4 us per timestep.  Inside the loop the level-3
    // kernel sets its priority by progress in the rounds, 0 to 2 (LLPF_ROUND_PRIO below); 3 stays with these phases.
    __builtin_amdgcn_s_setprio(3);
    const int f = blockIdx.y;
    const int tile = blockIdx.x;
    const int64_t Ns = b.Ns;
    const ModelD* md = models + f;
    FilterScal* sc = b.scal + f;
    const uint32_t stop_flag = *b.bank_flag;     // tested in res_head, after all other loads are in flight
    const int fb_flag = sc->fallback;
    if (threadIdx.x < 8) sh_tq[threadIdx.x] = 0;
    const uint64_t* __restrict__ qsrc = b.quanta + (size_t)f * Ns;
    const int64_t ib = (int64_t)tile * TILE + (int64_t)threadIdx.x * NORM_IPT;
    ulonglong2 qv[NORM_IPT / 2];
    int anc_ident_v = sc->anc_ident_s[b.anc_slot];            // this launch writes the other entry
    if (OWN_TABLE) {   // owner table of the output loop: cleared here, filled after the counts (res_owner_table)
        const uint4 z = {0u, 0u, 0u, 0u};
        reinterpret_cast<uint4*>(sh_own)[2 * threadIdx.x] = z;
        reinterpret_cast<uint4*>(sh_own)[2 * threadIdx.x + 1] = z;
    }
    double rt0 = 0.0, rt1 = 0.0;
// phase stamps (tools/dbg/timing_c2.sh): compiled in with DEVTOOLS=1 only — the test of a.dbg at the kernel's first instruction made
// every block wait for a scalar load of the argument block before it could request anything else
#ifdef LLPF_DEVTOOLS
#define LLPF_STAMP(i) if (a.dbg && threadIdx.x == 0 && f == 0) a.dbg[(size_t)tile * 8 + (i)] = wall_clock64()
#else
#define LLPF_STAMP(i) ((void)0)
#endif
    LLPF_STAMP(0);
    Model model;
    double y[NY];
    uint32_t key0_v = sc->k0, key1_v = sc->k1, sb_v = sc->step_base;
    const double c0_pre = md->dg.c0;                   // fetched with the other loads: the bound below must not wait for it
    // particle-independent terms (B u, the measurement row): their loads run while the head's vector loads are in flight
    auto prepare = [&]() {
        model.prepare(md, st.u + (size_t)f * st.u_stride, st.t_prop);
        const double* yf = st.y + (size_t)f * st.y_stride;
#pragma unroll
        for (int k = 0; k < NY; ++k) y[k] = (WEIGHT && st.has_y) ? yf[k] : 0.0;
        // Issued LAST, after everything the head itself waits for (accumulator words, tile sums: a few KB): the tile's quanta
        // are 8 MB over the whole launch, all blocks start at once, and loads return in order — issued first they kept every
        // head waiting 2.5 us for a burst that is only needed by the counts.  Likewise the generator's tables (for the loop).
#pragma unroll
        for (int k = 0; k < NORM_IPT / 2; ++k) qv[k] = *reinterpret_cast<const ulonglong2*>(qsrc + ib + 2 * k);
        if (!RBFAT) {
            const int t = (int)threadIdx.x;
            if (t < LLPF_RNG_SC_ENTRIES) { rt0 = LLPF_SIN64[t]; rt1 = LLPF_COS64[t]; }
            else if (t < LLPF_RNG_SC_ENTRIES + LLPF_RNG_LG_ENTRIES) { rt0 = LLPF_LOG_INVC[t - LLPF_RNG_SC_ENTRIES]; rt1 = LLPF_LOG_LNC[t - LLPF_RNG_SC_ENTRIES]; }
        }
    };
    static_assert(!SKIPW || (WEIGHT && ACC && !AUX && !ONE && !Model::RB), "the form without the weight store: merged schedule, several tiles");
    // SKIPW means that host/run_plan.hpp saw resample_threshold == 1 (RunForm::level): every step of the run resamples, none needs E2
    constexpr bool ALWAYS_RES = SKIPW;
    static_assert(!ALWAYS_RES || (WEIGHT && ACC && !AUX), "a launch that always resamples: the merged schedule's weighting form, never forced");
    constexpr bool LEAN_HEAD = LEAN && LLPF_LEAN_HEAD, LEAN_TAIL = LEAN && LLPF_LEAN_TAIL;
    const ResHead h = res_head<SRC_FILTER, false, decltype(prepare)&, SKIPW, LEAN_HEAD, NOMAX>(b, a, f, tile, sh, true, stop_flag, fb_flag, prepare);
    if (h.status) return;
    // Values of FilterScal fetched above with the head's loads but wanted only from here on.  FilterScal is written by this
    // kernel, so they are vector loads made uniform with v_readfirstlane — which the compiler otherwise places right behind the
    // loads, with a vmcnt wait BEFORE the head's own loads are issued (a second, serialized memory round trip at the start of
    // every block).  The asm pins the first use behind the head's barrier.
    asm volatile("" : "+v"(key0_v), "+v"(key1_v), "+v"(sb_v), "+v"(anc_ident_v));
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key0_v), key1 = __builtin_amdgcn_readfirstlane(key1_v);
    const uint32_t sb = __builtin_amdgcn_readfirstlane(sb_v);
    const int anc_ident_prev = __builtin_amdgcn_readfirstlane(anc_ident_v);
    if (!RBFAT) {      // the generator's tables -> LDS (one 16-byte LDS read per lookup instead of two global loads); the
        const int t = (int)threadIdx.x;     // barriers of the counts / the one below come before the loop reads them
        if (t < LLPF_RNG_SC_ENTRIES) { sh_rng_sc[2 * t] = rt0; sh_rng_sc[2 * t + 1] = rt1; }
        else if (t < LLPF_RNG_SC_ENTRIES + LLPF_RNG_LG_ENTRIES) { sh_rng_lg[2 * (t - LLPF_RNG_SC_ENTRIES)] = rt0; sh_rng_lg[2 * (t - LLPF_RNG_SC_ENTRIES) + 1] = rt1; }
    }
    LLPF_STAMP(1);
    // the items of the level-3 round (every other form: 0, its code untouched)
    constexpr int LR = ((LEAN && WEIGHT && ACC && !RBFAT) ? LLPF_LR_BITS : 0) | (NOMAX ? LLPF_LR_NOMAX : 0);
    // lean_acc_add forms no sum of squares and hands out no e: only where neither is wanted (LEAN: always resamples, no weighted means)
    constexpr int LR_ACC = LR & (LLPF_LR_QFIX | LLPF_LR_NANFLAG | LLPF_LR_CARRY);
    static_assert(LR == 0 || (LEAN && SKIPW), "the items of the lean round are level 3's");
    PropCtx<Model, NX, NY, WEIGHT, false, !RBFAT, !SKIPW, LR> pc{b, model, md, st, y, b.xcur + (size_t)f * NX * Ns, b.xnext + (size_t)f * NX * Ns,
                                      b.w + (size_t)f * Ns, b.w_next + (size_t)f * Ns, key0, key1, sb + st.step, a.ablate, 0.0, b.quanta_next + (size_t)f * Ns,
                                      RBFAT ? nullptr : sh_rng_lg, RBFAT ? nullptr : sh_rng_sc};
    double bz[NX];
    if constexpr ((LR & LLPF_LR_BZ) != 0) { model.input_term(bz); pc.bz = bz; }
    bool wnan = false;       // LLPF_LR_NANFLAG: WeightAcc::bad as a flag
    int32_t* anc = b.anc + (size_t)f * Ns;
    double bmax = -LLPF_INF;
    bool bad = false;

    // One loop over the outputs this block produces (the per-output body is instantiated once):
    //   resampling : outputs [c_start, c_end) from the ancestor counts, source = tile's owner of the output;
    //                the last tile also takes [c_end, M): thresholds >= bins[N], for which the reference leaves
    //                j[i] untouched (resample.jl:25-34) -> previous ancestor (identity if the last predict! did
    //                not resample)
    //   otherwise  : s.j .= 1:N, the tile's own particles (padding lanes included so that their weight stays -Inf)
    const bool res = ALWAYS_RES || ((h.dr || a.force) && h.tot != 0);
    // (tested where they are used, as ever: read once up here the two arguments stay in SGPRs across the whole kernel, which the forms
    // that do test them pay for in lanes)
#define LLPF_NEED_E2 (!ALWAYS_RES && st.need_e2 != 0)
#define LLPF_WANT_XM (!LEAN && st.want_xmean)
    int64_t first, last;
    int32_t c_end = 0;
    double l = 0.0;
    WeightAcc wacc;
    TileSum ts;
    wacc.init();
    ts.init();
    double xm[NX];
#pragma unroll
    for (int d = 0; d < NX; ++d) xm[d] = 0.0;
    uint64_t* tq_next = tileq_slot(b, st.parity, f);
    if (res) {
        int32_t c_start;
        if constexpr (!ACC) {
            // ResArgs::lazy_q (split schedule): the k_norm in front of this launch stored no quanta and `qsrc` is the filter's WEIGHTS — what the
            // speculative request above brought are the tile's raw log-weights, and their quanta are formed here, by k_norm's own expression
            // against the offset the head has just read back (the bound, or the maximum after a one-tile redo): identical integers.  A step
            // that does not resample (97 of 100 at the reference's threshold) thus moves neither the 8 bytes k_norm stored nor the 8 read here.
            if (a.lazy_q) {
#pragma unroll
                for (int k = 0; k < NORM_IPT / 2; ++k) {
                    qv[k].x = llpf_q64_unit(llpf_exp_le0(llpf_u2d(qv[k].x) - h.a), a.K);
                    qv[k].y = llpf_q64_unit(llpf_exp_le0(llpf_u2d(qv[k].y) - h.a), a.K);
                }
            }
        }
        if constexpr (LEAN_HEAD) res_counts<LLPF_RESAMPLE_SYSTEMATIC, true>(b, a, f, tile, h, qv, sh, c_start, c_end);
        else if (LEAN || b.strategy == LLPF_RESAMPLE_SYSTEMATIC) res_counts<LLPF_RESAMPLE_SYSTEMATIC>(b, a, f, tile, h, qv, sh, c_start, c_end);
        else if constexpr (!LEAN) res_counts<LLPF_RESAMPLE_STRATIFIED>(b, a, f, tile, h, qv, sh, c_start, c_end);
        first = c_start;
        last = (tile == b.P2 - 1) ? (int64_t)a.M : (int64_t)c_end;
        if (OWN_TABLE) res_owner_table(sh, sh, sh_own, c_start);
    } else if constexpr (!ALWAYS_RES) {
        l = head_log(h);
        first = (int64_t)tile * TILE;
        last = first + TILE;
        if (!RBFAT) __syncthreads();      // generator tables in LDS
    }
    {   // bound of the weights produced below: max of the previous (normalised) weights + the density's peak
        const double wmx = (ALWAYS_RES || res) ? b.log1N : (h.mtrue - h.a) - l;
        if constexpr (Model::RB) {     // peak of N(0, S) of the coming correct! (or of R2 when C == 0)
            const double c0w = md->rb_zeroC ? md->dg.c0 : (st.rb_corr + f)->dS.c0;
            pc.off = (WEIGHT && st.has_y) ? wmx + c0w : wmx;
        } else {
            pc.off = (WEIGHT && st.has_y) ? wmx + c0_pre : wmx;
        }
    }
    const double lN = -b.mlogN;
    const double aux_off = ((st.aux == 2) ? md->dg.c0 : 0.0) - lN;     // lambda - log N <= c0 - log N (lambda = 0 if y1 is missing)
    if (AUX) pc.off = aux_off;
    const double* lamp = AUX ? b.lam + (size_t)f * Ns : nullptr;
    const int32_t tbase = (int32_t)(first >> 10);
    LLPF_STAMP(2);
#ifdef LLPF_DEVTOOLS
    if (a.dbg && threadIdx.x == 0 && f == 0) a.dbg[(size_t)tile * 8 + 5] = (uint64_t)(last - first);
    // where the block ran: HW_REG_HW_ID (register 4: cu_id [11:8], sh_id [12], se_id [15:13]) and HW_REG_XCC_ID (register 20: [3:0]), all 32 bits of
    // each, so that tools/dbg/timing_report.py can give the stagger of the blocks that shared a CU
    if (a.dbg && threadIdx.x == 0 && f == 0) {
        a.dbg[(size_t)tile * 8 + 6] = (uint64_t)__builtin_amdgcn_s_getreg(4 | (31 << 11));
        a.dbg[(size_t)tile * 8 + 7] = (uint64_t)__builtin_amdgcn_s_getreg(20 | (31 << 11));
    }
#endif
    const uint32_t tile0 = (uint32_t)tile * TILE, ulast = (uint32_t)last, ucend = (uint32_t)c_end;
    // end of the outputs that have an owner in this tile; [umain, ulast) is the last tile's [c_end, M) of a resampling step, else empty
    // PEEL: the merged-schedule kernels.  The run-time-split Rao-Blackwellized kernels keep the test inside their one loop (a second copy
    // of their body costs them 16 bytes of stack), and so do the split-schedule forms: their loops do not wait for their gathers, and with
    // the second loop they measured 1.1 % (C4 share) and 1.5 % (N = 1.6e7, threshold 1) slower (EXPERIMENTS: the output loop's rounds)
    constexpr bool PEEL = WEIGHT && ACC && !RBFAT;
    const uint32_t umain = (res && PEEL) ? (ucend < ulast ? ucend : ulast) : ulast;
    // the map of the rounds' priority by progress: the level-3 kernel alone (the other forms keep one priority for the loop, their code untouched)
    constexpr int LOOP_PRIO = (LEAN && PEEL) ? LLPF_LOOP_PRIO : 0;
    __builtin_amdgcn_s_setprio(0);
    // tile-local source of output o (< c_end): the owner table, the descent beyond it
    auto owner_of = [&](uint32_t o) -> uint32_t {
#ifdef LLPF_DEVTOOLS
        if (a.ablate & 2) return (o - (uint32_t)first) & (TILE - 1);
#endif
        const uint32_t idx = o - (uint32_t)first;
        return (OWN_TABLE && idx < (uint32_t)OWN_CAP) ? sh_own[idx] - 1u : (uint32_t)res_owner(sh.cl, (int32_t)o);
    };
    // The output loop: source of output o (owner table / previous ancestor / o itself), its previous weight (log(1/N) after a
    // resampling; lambda - log N in the auxiliary filter's second half; else the lazily normalised stored weight: w .-= offset,
    // w .-= log(sum)), propagate [+ weight], exp-sum / quanta / tile-sum accumulation.  Written once, instantiated per value of
    // the block-uniform resample flag where that measured faster (split-schedule and Rao-Blackwellized kernels: each version
    // keeps only its own uniform values live; the merged single-filter kernel is 0.3 us faster with ONE loop and the flag
    // tested inside).
    // The rounds of [c_end, M) are a loop of their own behind the others (STALE = 1; 0: the rounds with an owner; 2: either, tested per
    // round): their source is a LOAD (the previous ancestor), the loop's only other vector load, and with it in the common round the
    // compiler's wait-count pass drained the vector-memory counter four times at the top of EVERY round — stores count in vmcnt on
    // gfx950, so each round's owner lookup and gather waited for the previous round's write-through stores to be acknowledged
    // (profiles/loop_chain_isa.txt).  A thread still visits its outputs in increasing order (TileSum sees the same sequence), and the
    // body is the same text.
    // SKIPA: only the rounds of [c_end, M) store their ancestor (a compile-time choice: a test in the loop costs more than the store)
#ifdef LLPF_DEVTOOLS   /* LLPF_ABLATE bit 4: the same behind a run-time test, and without the entry kept behind the loop (results invalid) */
#define LLPF_ANC_KEPT(STALE) ((STALE) == 1 || (!SKIPA && !(a.ablate & 16)))
#else
#define LLPF_ANC_KEPT(STALE) ((STALE) == 1 || !SKIPA)
#endif
    // Priority by progress (LOOP_PRIO: level 3 only; shared/llpf_loop_prio.h): inside the loop every wave used to run at priority 0, that is by
    // age — the wave of the block dispatched first on a CU ran all its rounds first, the youngest block's wave ran its rounds last and alone
    // on its SIMD.  Here a wave sets its priority at the top of each round with an owner from the rounds it still has to do, this one
    // included: what is behind in rounds wins arbitration, equal progress falls back to age, and the waves of a SIMD pass the loop side by
    // side.  The count is the wave's first lane's (the lowest output of the wave, so the most rounds of its lanes, and exactly the
    // rounds the wave runs): scalar arithmetic on first, umain and that lane's thread index (one v_readfirstlane in front of the loop),
    // counted down in an SGPR; s_setprio takes an immediate, so a round branches onto one of up to four.  No vector instruction and no
    // VGPR in the round, no arithmetic, store or order changed.  Every wave's last round runs at priority 0, so the rounds of
    // [c_end, M) behind it do too, and the tail raises it to 3 as ever.
    // Kept: map A (C2 17.64 -> 16.71 us per timestep, map B 16.89; the last block of a launch ends at 16.5 instead of 17.9 - 18.9 us, the
    // loop exits of a CU's four blocks are 1.9 instead of 4.7 us apart: EXPERIMENTS, profiles/loop_prio_*.txt).
#define LLPF_ROUNDS_LEFT \
    int rounds_left = 0; \
    if constexpr (LOOP_PRIO != 0) { \
        const uint32_t o0 = (uint32_t)first + (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x);      /* the first lane's output: first, umain and it are scalars */ \
        rounds_left = o0 < umain ? (int)((umain - o0 + (uint32_t)(BLOCK - 1)) / (uint32_t)BLOCK) : 0; \
    }
#define LLPF_ROUND_PRIO(STALE) \
        if constexpr (LOOP_PRIO != 0 && (STALE) == 0) { \
            switch (llpf_loop_prio(LOOP_PRIO, rounds_left)) { \
                case 3: __builtin_amdgcn_s_setprio(3); break; \
                case 2: __builtin_amdgcn_s_setprio(2); break; \
                case 1: __builtin_amdgcn_s_setprio(1); break; \
                default: __builtin_amdgcn_s_setprio(0); break; \
            } \
            --rounds_left; \
        }
#define LLPF_OUTPUT_ROUNDS(RESX, NTLX, STALE, OEND) \
_Pragma("unroll 1") \
    for (; o < (OEND); o += BLOCK) { \
        LLPF_ROUND_PRIO(STALE) \
        uint32_t src = o; \
        double wprev = b.log1N; \
        if (RESX) { \
            if ((STALE) == 0 || ((STALE) == 2 && o < ucend)) src = tile0 + owner_of(o); \
            else src = anc_ident_prev ? o : (uint32_t)ld_off(anc, o << 2); \
            if (LLPF_ANC_KEPT(STALE)) Mem<LLPF_STCOH0>::st_off(anc, o << 2, (int32_t)src); \
            if (AUX) wprev = ld_off(lamp, o << 3) - lN; \
        } else if (AUX) { \
            wprev = ld_off(lamp, o << 3) - lN; \
        } else if (WEIGHT && !ALWAYS_RES) { \
            wprev = (ld_off(pc.w, o << 3) - h.a) - l; \
        } \
        double xs[NX]; \
        const double wv = pc.template one<LLPF_RESPROP_ST, NTLX>(src, o, wprev, bad, xs); \
        if constexpr (!NOMAX) bmax = llpf_fmax(bmax, wv); \
        LLPF_OUTPUT_ACC(o, wv, xs) \
    }
#ifdef LLPF_DEVTOOLS   /* LLPF_ABLATE bit 6, level 3 only (K >= 33 there: launch_resprop_t): one shift for the quantum and no NaN count (what items 1 and 2 of the lean round can save at most; results invalid) */
#define LLPF_ACC_ADD(wv, e) ((LEAN && (a.ablate & 64)) ? ablated_acc_add(wacc, wv, pc.off, st.K) : (LR_ACC != 0 ? lean_acc_add<LR_ACC>(wacc, wnan, wv, pc.off, st.K) : wacc.add(wv, pc.off, st.K, LLPF_NEED_E2, &e)))
#else
#define LLPF_ACC_ADD(wv, e) (LR_ACC != 0 ? lean_acc_add<LR_ACC>(wacc, wnan, wv, pc.off, st.K) : wacc.add(wv, pc.off, st.K, LLPF_NEED_E2, &e))
#endif
#define LLPF_OUTPUT_ACC(o, wv, xs) \
        if (WEIGHT && ACC) { \
            double e; \
            const uint64_t q = LLPF_ACC_ADD(wv, e); \
            Mem<LLPF_STCOH0>::st_off(pc.qnext, (o) << 3, q); \
            ts.add(o, q, sh_tq, tq_next, tbase); \
            if (LLPF_WANT_XM) { \
_Pragma("unroll") \
                for (int d = 0; d < NX; ++d) xm[d] = xm[d] + xs[d] * e; \
            } \
        }
#define LLPF_OUTPUT_STALE \
    if (umain < ulast) { LLPF_OUTPUT_ROUNDS(true, false, 1, ulast) }
#define LLPF_OUTPUT_LOOP(RESX, NTLX) { \
    uint32_t o = (uint32_t)first + threadIdx.x; \
    LLPF_ROUNDS_LEFT \
    LLPF_OUTPUT_ROUNDS(RESX, NTLX, PEEL ? 0 : 2, umain) \
    if (PEEL && (RESX)) { LLPF_OUTPUT_STALE } \
}
    // The same loop with the sources of LLPF_RESPROP_PF consecutive rounds requested together, for the split-schedule form — the kernel of
    // filters and banks beyond 3 M particles, whose states come from HBM instead of the Infinity Cache.  Worth 2 % at depth 2 and
    // nothing beyond (depth 4 is slower): the loop of such a launch does not wait for its gathers — what moved it was the store policy
    // (k_resprop_split.hip), which this loop takes per kind of step: LLPF_RESPROP_ST on a resampling step, LLPF_RESPROP_ST_ID on a step
    // whose outputs read their own index.  The per-output arithmetic and its order are untouched; the ancestors are stored behind the
    // loads (stores and loads share a counter).
#define LLPF_OUTPUT_LOOP_PF(RESX) \
_Pragma("unroll 1") \
    for (uint32_t ob = (uint32_t)first + threadIdx.x; ob < ulast; ob += LLPF_RESPROP_PF * BLOCK) { \
        uint32_t srcs[LLPF_RESPROP_PF]; \
        double wps[LLPF_RESPROP_PF], xps[LLPF_RESPROP_PF][NX]; \
_Pragma("unroll") \
        for (int k = 0; k < LLPF_RESPROP_PF; ++k) { \
            const uint32_t o = ob + (uint32_t)k * BLOCK; \
            srcs[k] = o; \
            if (RESX && o < ulast) { \
                if (o < ucend) srcs[k] = tile0 + owner_of(o); \
                else srcs[k] = anc_ident_prev ? o : (uint32_t)ld_off(anc, o << 2); \
            } \
        } \
_Pragma("unroll") \
        for (int k = 0; k < LLPF_RESPROP_PF; ++k) { \
            const uint32_t o = ob + (uint32_t)k * BLOCK; \
            wps[k] = b.log1N; \
            if (o < ulast) { \
                pc.template fetch<!(RESX) && LLPF_RESPROP_LD_ID>(srcs[k], xps[k]); \
                if (!(RESX) && WEIGHT) wps[k] = (ld_off(pc.w, o << 3) - h.a) - l; \
            } \
        } \
_Pragma("unroll") \
        for (int k = 0; k < LLPF_RESPROP_PF; ++k) { \
            const uint32_t o = ob + (uint32_t)k * BLOCK; \
            if (o < ulast) { \
                if (RESX) Mem<LLPF_STCOH0>::st_off(anc, o << 2, (int32_t)srcs[k]); \
                double xs[NX]; \
                const double wv = pc.template one_x<(RESX) ? LLPF_RESPROP_ST : LLPF_RESPROP_ST_ID>(xps[k], o, wps[k], bad, xs); \
                bmax = llpf_fmax(bmax, wv); \
            } \
        } \
    }
    // A step that does not resample, split-schedule form: output o reads index o, so a thread takes TWO ADJACENT outputs and every plane
    // is read and written 16 bytes per lane — three loads and three stores per pair instead of six and six.  With 8-byte accesses this
    // loop was bound by neither issue nor bandwidth but by the number of memory instructions in flight: cut to a third of its vector
    // instructions (the tile-loop experiment, EXPERIMENTS 6.12) it took the same time, 4.9 TB/s.  Per-output arithmetic and counters
    // untouched (PropCtx::one_x with STP = -1 returns what it would have stored).  The nontemporal forms of both (LLPF_RESPROP_LD_ID, _ST_ID) are
    // taken when the host says so (ResArgs::nt_id): from ~7 M particles on; a working set the size of the Infinity Cache prefers plain accesses
    // (N = 3.3e6 / 4e6 at threshold 0.1: 47.0 / 55.1 us plain, 52.6 / 62.1 nontemporal; 8e6: 109.0 / 108.0; 1.6e7: 209.3 / 202.4).  (The same pairing for the steps that DO resample — adjacent
    // outputs, 16-byte stores of both states, weights and ancestors — is 7.6 % slower than two rounds a block apart, and so is that loop with
    // only its STORES paired (neighbouring lanes exchange halves through quad_perm, the gathers keep their spread): 9 % slower — 16-byte
    // plain stores beside a gather cost more than twice as many 8-byte ones.  Both pairs of a thread requested before the first is computed:
    // no better, 169.2 / 170.0 us on the C4 share.  profiles/r06_paired_outputs_ab.txt.)
#define LLPF_OUTPUT_LOOP_ID2(LDNT, STNT) \
_Pragma("unroll 1") \
    for (uint32_t o2 = (uint32_t)first + 2u * threadIdx.x; o2 < ulast; o2 += 2u * BLOCK) { \
        typedef double __attribute__((ext_vector_type(2))) d2_t; \
        d2_t xv[NX], wv2 = {b.log1N, b.log1N}; \
_Pragma("unroll") \
        for (int d = 0; d < NX; ++d) { \
            const d2_t* src_ = reinterpret_cast<const d2_t*>(reinterpret_cast<const char*>(pc.xc + (size_t)d * Ns) + (o2 << 3)); \
            xv[d] = (LDNT) ? __builtin_nontemporal_load(src_) : *src_; \
        } \
        if (WEIGHT) wv2 = *reinterpret_cast<const d2_t*>(reinterpret_cast<const char*>(pc.w) + (o2 << 3)); \
        double xp0[NX], xp1[NX], xs0[NX], xs1[NX]; \
_Pragma("unroll") \
        for (int d = 0; d < NX; ++d) { xp0[d] = xv[d].x; xp1[d] = xv[d].y; } \
        const double wp0 = WEIGHT ? (wv2.x - h.a) - l : b.log1N, wp1 = WEIGHT ? (wv2.y - h.a) - l : b.log1N; \
        const double w0 = pc.template one_x<-1>(xp0, o2, wp0, bad, xs0); \
        const double w1 = pc.template one_x<-1>(xp1, o2 + 1u, wp1, bad, xs1); \
        bmax = llpf_fmax(bmax, w0); \
        bmax = llpf_fmax(bmax, w1); \
_Pragma("unroll") \
        for (int d = 0; d < NX; ++d) { \
            d2_t v_; v_.x = xs0[d]; v_.y = xs1[d]; \
            d2_t* dst_ = reinterpret_cast<d2_t*>(reinterpret_cast<char*>(pc.xn + (size_t)d * Ns) + (o2 << 3)); \
            if (STNT) __builtin_nontemporal_store(v_, dst_); else *dst_ = v_; \
        } \
        if (WEIGHT) { \
            d2_t v_; v_.x = w0; v_.y = w1; \
            d2_t* dst_ = reinterpret_cast<d2_t*>(reinterpret_cast<char*>(pc.wn) + (o2 << 3)); \
            if (STNT) __builtin_nontemporal_store(v_, dst_); else *dst_ = v_; \
        } \
    }
    constexpr bool PREFETCH = LLPF_RESPROP_PF > 1 && !(WEIGHT && ACC) && !Model::RB && !AUX;
    if constexpr (WEIGHT && ACC && !Model::RB) { LLPF_OUTPUT_LOOP(res, false) }
    else if constexpr (PREFETCH) { if (res) { LLPF_OUTPUT_LOOP_PF(true) } else if (LLPF_RESPROP_ID2) { if (a.nt_id) { LLPF_OUTPUT_LOOP_ID2(LLPF_RESPROP_LD_ID != 0, LLPF_RESPROP_ST_ID == 2) } else { LLPF_OUTPUT_LOOP_ID2(false, false) } } else { LLPF_OUTPUT_LOOP_PF(false) } }
    else if (res) { LLPF_OUTPUT_LOOP(true, false) }
    else { LLPF_OUTPUT_LOOP(false, (LLPF_RESPROP_LD_ID != 0)) }
#undef LLPF_OUTPUT_LOOP
#undef LLPF_OUTPUT_ROUNDS
#undef LLPF_ROUNDS_LEFT
#undef LLPF_ROUND_PRIO
#undef LLPF_OUTPUT_STALE
#undef LLPF_ANC_KEPT
#undef LLPF_OUTPUT_ACC
#undef LLPF_ACC_ADD
#undef LLPF_OUTPUT_LOOP_PF
#undef LLPF_OUTPUT_LOOP_ID2
    if constexpr (SKIPA) {
        // the one entry the next launch may read (its rounds of [c_end, M)): the ancestor of output M - 1, by the block that owns it
        static_assert(PEEL, "SKIPA: the rounds with and without an owner are separate loops");
        if (res && ucend == (uint32_t)a.M && (uint32_t)first < ucend && threadIdx.x == 0)
            Mem<LLPF_STCOH0>::st_off(anc, (ucend - 1u) << 2, (int32_t)(tile0 + owner_of(ucend - 1u)));
    }
    if (WEIGHT && ACC) ts.flush(sh_tq, tq_next, tbase);
    __builtin_amdgcn_s_setprio(3);
    LLPF_STAMP(3);
#ifdef LLPF_DEVTOOLS   /* LLPF_ABLATE bit 5: the tail without its accumulator atomics (acc_max, acc_add_u128): what they cost at most; results invalid */
#define LLPF_NO_TAIL_ATOMICS ((a.ablate & 32) != 0)
#define LLPF_TAIL_ABLATE a.ablate      /* level 4: bit 5 the same, bit 7 its sums on 32 lines (block_flush_sums) */
#else
#define LLPF_NO_TAIL_ATOMICS false
#define LLPF_TAIL_ABLATE 0
#endif
    if constexpr ((LR & LLPF_LR_NANFLAG) != 0) wacc.bad = wnan ? 1u : 0u;
    if constexpr (LEAN_TAIL) {
        // The tail in ONE barrier (block_flush, as in k_step<..., MARKS>): every wave reduces its maximum, NaN flag and exp-sums and leaves
        // one LDS row; the threads' tile sums went to sh_tq in front of it (ts.flush above); behind the barrier thread 0 combines the rows and
        // issues the accumulator atomics while threads 0..7 add sh_tq to the global tile sums.  A block that owns no outputs (first == last:
        // a tile behind a very heavy one) contributes the maximum -Inf, no NaN flag and no sum, as in the levels below.
        if constexpr (NOMAX) block_flush_sums(b.acc + (size_t)f * ACC_WORDS, st.parity, wacc, sm_fl, LLPF_TAIL_ABLATE);
        else block_flush(b.acc + (size_t)f * ACC_WORDS, st.parity, bmax, bad, wacc, true, false, sm_fl, LLPF_NO_TAIL_ATOMICS);
        if (threadIdx.x < 8 && sh_tq[threadIdx.x])
            atomicAdd(reinterpret_cast<unsigned long long*>(tq_next + tbase + threadIdx.x), (unsigned long long)sh_tq[threadIdx.x]);
        if (tile == 0 && threadIdx.x == 0) {
            sc->xm_parts = b.P2;
            sc->off_slot[st.parity] = pc.off;
            sc->exact_slot[st.parity] = 0;
            sc->e2v_slot[st.parity] = st.need_e2;
            sc->u_slot[st.parity] = llpf_uniform_step(sb + st.next_step, LLPF_STREAM_RESAMPLE, sc->k0, sc->k1);
        }
        // No closing barrier: nothing behind this point reads what another thread of the block wrote — the bookkeeping below is one thread's
        // read-modify-write of fields that no other thread of the launch touches, and LDS is not read again.
    } else {      // every other form: the tail as it was (its lines left where they stood)
    if (WEIGHT) {
        const double r = block_max(bmax, sm_max);
        const int anybad = __syncthreads_or(bad ? 1 : 0);
        if (threadIdx.x == 0 && !LLPF_NO_TAIL_ATOMICS) acc_max(b.acc + (size_t)f * ACC_WORDS, st.parity, r, anybad != 0);
        int exact = 0;
        if constexpr (ACC && ONE) {
            // This block is the whole filter (one tile): make the bound test of the coming head here and, if it fails,
            // redo the sums in exact-max form at once (same arithmetic as k_norm's exact form; the head is told through
            // exact_slot).  Banks of many small filters otherwise pay a host round trip at nearly every timestep.
            const llpf_u128 sw = wave_sum_u128(wacc.S);
            if ((threadIdx.x & 63) == 0) { sm_acc[threadIdx.x >> 6][0] = sw.lo; sm_acc[threadIdx.x >> 6][1] = sw.hi; }
            __syncthreads();
            llpf_u128 tot = {sm_acc[0][0], sm_acc[0][1]};
            for (int k = 1; k < BLOCK / 64; ++k) { const llpf_u128 t1 = {sm_acc[k][0], sm_acc[k][1]}; tot = llpf_u128_add(tot, t1); }
            __syncthreads();
            if (anybad || tot.hi < ((uint64_t)1 << 22)) {
                exact = 1;
                const double mx = anybad ? llpf_u2d(0x7ff8000000000000ULL) : r;
                wacc.init();
                ts.init();
                if (threadIdx.x < 8) sh_tq[threadIdx.x] = 0;
#pragma unroll
                for (int d = 0; d < NX; ++d) xm[d] = 0.0;
                __syncthreads();
#pragma unroll 1
                for (uint32_t o = (uint32_t)first + threadIdx.x; o < ulast; o += BLOCK) {
                    const double wv = ld_off(pc.wn, o << 3);
                    double e;
                    const uint64_t q = wacc.add(wv, mx, st.K, LLPF_NEED_E2, &e);
                    st_off(pc.qnext, o << 3, q);
                    ts.add(o, q, sh_tq, tq_next, tbase);
                    if (LLPF_WANT_XM) {
#pragma unroll
                        for (int d = 0; d < NX; ++d) xm[d] = xm[d] + ld_off(pc.xn + (size_t)d * Ns, o << 3) * e;
                    }
                }
                ts.flush(sh_tq, tq_next, tbase);
            }
        }
        if (ACC) {
            wacc.flush(b.acc + (size_t)f * ACC_WORDS, st.parity, LLPF_NEED_E2, sm_acc, LLPF_NO_TAIL_ATOMICS);
            __syncthreads();
            if (threadIdx.x < 8 && sh_tq[threadIdx.x])
                atomicAdd(reinterpret_cast<unsigned long long*>(tq_next + tbase + threadIdx.x), (unsigned long long)sh_tq[threadIdx.x]);
            if (LLPF_WANT_XM) block_store_xm<NX>(xm, xmpart_slot(b, st.parity, f) + (size_t)tile * MAXD, sm_x);
        }
        if (tile == 0 && threadIdx.x == 0) {
            if (AUX) {     // the weights just written are final values (no pending normalisation); aux_off bounds them
                sc->norm_pending = 0;
                sc->uniform = 0;
                sc->wmax = aux_off;
            }
            if (ACC) sc->xm_parts = b.P2;
            sc->off_slot[st.parity] = pc.off;
            sc->exact_slot[st.parity] = exact;
            sc->e2v_slot[st.parity] = st.need_e2;
            sc->u_slot[st.parity] = llpf_uniform_step(sb + st.next_step, LLPF_STREAM_RESAMPLE, sc->k0, sc->k1);
        }
    }
    __syncthreads();
    }
    LLPF_STAMP(4);
#undef LLPF_STAMP
#undef LLPF_NO_TAIL_ATOMICS
#undef LLPF_TAIL_ABLATE
#undef LLPF_NEED_E2
#undef LLPF_WANT_XM
    if (tile == b.P2 - 1 && threadIdx.x == 0) {        // bookkeeping of this predict! (by the only block that reads anc_ident)
        const int r = res ? 1 : 0;
        sc->anc_ident_s[b.anc_slot ^ 1] = r ? 0 : 1;
        sc->last_resampled = r;
        sc->resample_count += r;
    }
}
