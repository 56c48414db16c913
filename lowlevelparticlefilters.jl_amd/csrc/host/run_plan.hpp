// host/run_plan.hpp — the form of a run as a value: which launches a trajectory loop consists of (RunPlan, decided once, in front
// of the first launch, from the facts of the bank, the requested outputs and the environment) and the host-side state in which each of
// its timesteps runs (StepState).  No device, no Bank, no HIP call: tests/run_plan_host.cpp builds it with a host compiler alone.
// host/run.hpp fills a RunFacts, enqueues what the plan says and keys its captured graphs by the plan's form (Bank::RunGraph).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "../../../include/llpf.h"

// The switches of the environment, parsed.  -1: not set (the rule decides).
struct RunSwitches {
    int unfused = -1, source_fx = -1, nt_id = -1;      // LLPF_UNFUSED, LLPF_SOURCE_FX, LLPF_NT_ID = 0/1
    int schedule = -1;                                 // LLPF_SCHEDULE: 1 for "merged", 0 for anything else (the split schedule)
    int lazy_q = -1, skip_w = -1, graph = -1;          // LLPF_LAZY_Q=0: the stored form; LLPF_SKIP_W=0: the storing form; LLPF_GRAPH=0: every run is enqueued
    int skip_anc = -1;                                 // LLPF_SKIP_ANC=0: a run without the weight store still stores every ancestor
    int lean = -1;                                     // LLPF_LEAN=0: such a run keeps the kernel that tests the strategy and the means at run time
    int skip_max = -1;                                 // LLPF_SKIP_MAX=0: every level-3 launch of such a run leaves its running maximum, as the run's last one does
    int ablate = 0;                                    // LLPF_ABLATE (DEVTOOLS builds)
    bool debug_timing = false;                         // LLPF_DEBUG_TIMING=k: the fused launch of step k leaves its per-tile clock readings behind; no graphs
    int64_t debug_step = 0;
};
static inline int env_flag(const char* v) { return v ? (atoi(v) != 0 ? 1 : 0) : -1; }
// Read on every run, except LLPF_ABLATE, LLPF_DEBUG_TIMING and LLPF_GRAPH: once per process.
static inline RunSwitches read_run_switches() {
    static const char* abl_env = getenv("LLPF_ABLATE");
    static const char* dbg_env = getenv("LLPF_DEBUG_TIMING");
    static const char* graph_env = getenv("LLPF_GRAPH");
    RunSwitches s;
    s.unfused = env_flag(getenv("LLPF_UNFUSED"));
    s.source_fx = env_flag(getenv("LLPF_SOURCE_FX"));
    const char* sch = getenv("LLPF_SCHEDULE");
    s.schedule = sch ? (strcmp(sch, "merged") == 0 ? 1 : 0) : -1;
    s.nt_id = env_flag(getenv("LLPF_NT_ID"));
    s.lazy_q = env_flag(getenv("LLPF_LAZY_Q"));
    s.skip_w = env_flag(getenv("LLPF_SKIP_W"));
    s.skip_anc = env_flag(getenv("LLPF_SKIP_ANC"));
    s.lean = env_flag(getenv("LLPF_LEAN"));
    s.skip_max = env_flag(getenv("LLPF_SKIP_MAX"));
    s.graph = env_flag(graph_env);
    s.ablate = abl_env ? atoi(abl_env) : 0;
    s.debug_timing = dbg_env != nullptr;
    s.debug_step = dbg_env ? atoll(dbg_env) : 0;
    return s;
}

struct RunFacts {
    // the bank
    int model_id = 0, nx = 0, F = 0, P2 = 0, strategy = 0;
    int64_t Ns = 0;
    double thr = 1.0;             // resample_threshold
    int traits = 0;               // LLPF_TRAIT_* of a run-time compiled model (0 for the built-in ones, -1 for an unknown id)
    bool fx_supported = false;    // resample_fx_supported(model, nx, ny, strategy)
    // the outputs asked for (hist: any of x_hist / w_hist / we_hist)
    bool hist = false, xmean = false, xcov = false, xquant = false, ll_steps = false, multi = false;
    // the handle
    bool profiling = false;
    int64_t T = 1;
    double surv_frac = -1.0;      // Bank::surv_frac
    bool use_fx = true;           // Bank::use_fx
    RunSwitches sw;
};

// What the fused launches of a merged run at resample_threshold 1 leave out — all of them but the exact redo of a failed bound test and
// the run's last launch (launch_level).  Ordered: each level is the one below it and one thing more.  Plain ints, so that the kernel's
// template argument and ResArgs::level are the same values (kernels/resprop.hpp).  The kernel relies on this: a level above RUN_STORES
// holds no arm for a step that does not resample and accumulates no sum of squares — it is planned at threshold exactly 1 and nowhere else.
enum RunLevel : int {
    RUN_STORES = 0,           // weights and ancestors are stored
    RUN_SKIP_W = 1,           // no weights are stored
    RUN_SKIP_ANC = 2,         // ... and no ancestor but output M - 1's
    RUN_LEAN = 3,             // ... by the kernel for systematic resampling without weighted means
    RUN_NO_MAX = 4,           // ... which leaves and reads no running maximum.  The level of single launches only (launch_level with a
                              // plan): a plan's level is at most RUN_LEAN, and RunKey::skip_max says whether its launches may take this one
};
// LLPF_SKIP_MAX=0 (compile time): no launch is ever RUN_NO_MAX, and the kernel is not built (kernels/resprop.hpp)
#ifndef LLPF_SKIP_MAX
#define LLPF_SKIP_MAX 1
#endif

// Everything a captured launch sequence depends on besides its buffers, its length and the entry state: the key of a captured graph
// holds one and compares it as a whole (Bank::RunGraph), so a switch added here is part of the key without further ado.  Plain ints
// (0/1 where the name is a yes/no), no padding: equality is equality of the bytes.
struct RunForm {
    int unfused;              // balanced form (ancestors to HBM, then a uniform propagate) instead of the fused launch
    int merged;               // exp-sums / quanta formed inside the weighting phase (else: a streaming k_norm launch per step)
    int acc_in_weighting;     // ... and whether the weighting launches form sums at all
    int no_bound;             // a likelihood without a bound: every step in the exact-max form
    int fx_capable;           // the balanced form of a model whose dynamics are worth a table: the launches count surviving sources
    int source_fx;            // f(x_j) once per surviving source in the resampling launch (kernels/resfx.hpp)
    int lazy_run;             // split schedule, fused: k_norm stores no quanta, two weight buffers
    int level;                // RunLevel of the run's fused launches (launch_level() gives each launch's own)
    int nt_id;                // nontemporal accesses on the steps that do not resample
    int want_xm;              // weighted means out of the normalise / weighting kernels
    int xm_launch;            // weighted means by a k_wmean launch per step (per-particle covariance)
    int k_pp0;                // first step of a lazy run that alternates between the two weight buffers
    int ablate;
    int ll_steps, multi, xcov, xquant;      // outputs and input layout the launch arguments depend on
    bool operator==(const RunForm& o) const { return memcmp(this, &o, sizeof(RunForm)) == 0; }
};
static_assert(std::has_unique_object_representations<RunForm>::value, "RunForm is compared bytewise: ints only, no padding");

// ... and what was decided since and is part of the key as well (RunForm keeps its seventeen ints).  Bank::RunGraph holds a RunKey.
struct RunKey : RunForm {
    int skip_max;             // the level-3 launches that another launch with a weighting phase follows are RUN_NO_MAX (launch_level)
    using RunForm::operator==;      // (against a plain RunForm: the form alone)
    bool operator==(const RunKey& o) const { return RunForm::operator==(o) && skip_max == o.skip_max; }
};

struct RunPlan : RunKey {
    bool use_graph;           // the asynchronous loop as a captured graph (replayed when its key is seen again)
    bool use_fx;              // Bank::use_fx after this run's look at surv_frac
};

static inline RunPlan make_run_plan(const RunFacts& f) {
    const RunSwitches& s = f.sw;
    RunPlan p{};
    const bool rbm = f.model_id == LLPF_MODEL_RB_LINEAR;
    const bool rbfull = f.model_id == LLPF_MODEL_RB_BILINEAR;     // per-particle covariance: its own step kernel, balanced form, exp-sums by k_norm
    const bool user_model = f.model_id >= LLPF_MODEL_USER_BASE;   // run-time compiled model: only its k_step exists
    const int64_t FNs = (int64_t)f.F * f.Ns;
    // Fused (one launch: finalize + resample + propagate + weight, a block propagates the outputs of its own source
    // tile) or balanced form (ancestors to HBM, then a uniform propagate).  The fused form saves a launch and the
    // ancestor round trip but its propagate work follows the weight distribution; models whose dynamics dominate the
    // timestep (quad-tank RK4: 32 fp64 sqrt per particle) and whose ESS is small run faster balanced (measured 69 vs
    // 121 us per timestep at N = 1e6), the linear-Gaussian model faster fused.  LLPF_UNFUSED=0/1 overrides.
    // ... and so does the linear-Gaussian model from three states on (measured at N = 1e6 on model-simulated data, tools/bench_nx.py:
    // nx 2 fused 21.1 / balanced 24.8 us per timestep, nx 3 33.8 / 28.8, nx 4 38.2 / 30.5 — the fused kernel drops to three waves per SIMD there)
    const bool heavy_dynamics = f.model_id == LLPF_MODEL_QUADTANK_RK4 || (f.model_id == LLPF_MODEL_LINEAR_GAUSSIAN && f.nx >= 3);
    // residual resampling produces unsorted ancestors (copies first, multinomial draws after): always the balanced form
    const bool residual = f.strategy == LLPF_RESAMPLE_RESIDUAL;
    // (xcov: the covariance is taken from the state between correct! and predict!, which only the balanced form leaves in memory)
    p.unfused = user_model || rbfull || f.hist || residual || f.xcov || f.xquant || (s.unfused >= 0 ? s.unfused != 0 : heavy_dynamics);
    // Models whose dynamics are worth a table: the resampling launch evaluates f(x_j) once per surviving source and leaves run-start marks,
    // the step kernel gathers (kernels/resfx.hpp).  LLPF_SOURCE_FX=0 takes the round-3 form (ancestors to HBM, f per distinct ancestor of a block).
    // Which of the two pays depends on how many sources survive a resampling — every f(x) of the source-side form makes a round trip
    // through HBM.  Quad-tank, N = 1e6, us per timestep (tools/dbg/qt_regimes.py; EXPERIMENTS.md 4.13): 0.8 % distinct ancestors
    // (BASELINE C3) 31.7 source-side / 36.3 per output, 4.9 % 35.1 / 36.0, 10.5 % 39.6 / 37.2, 24.6 % 47.0 / 38.9, 71 % 54.0 / 47.2.
    // Both launches count the sources whose f the step needed (BankDev::surv, per tile); the host switches the NEXT run's form with a
    // hysteresis (below 5 % -> source-side, above 8 % -> per output).  A handle's first run takes the source-side form.
    // LLPF_SOURCE_FX=0/1 pins it.
    p.fx_capable = p.unfused && f.fx_supported;
    p.use_fx = f.use_fx;
    if (p.fx_capable && f.surv_frac >= 0.0) { if (f.surv_frac < 0.05) p.use_fx = true; else if (f.surv_frac > 0.08) p.use_fx = false; }
    p.source_fx = p.fx_capable && (s.source_fx >= 0 ? s.source_fx != 0 : p.use_fx);
    // Where the exp-sums / quanta of freshly computed weights are formed (identical results either way): inside the
    // weighting phase (one launch per timestep: best when one filter of ~1e6 particles cannot fill the chip and the
    // dependent-launch latency dominates) or by a streaming k_norm launch in bound form (the fused kernel then keeps
    // its registers for the propagate and runs at higher occupancy: best when many filters saturate the SIMDs).
    // Measured on MI355X: C2 single filter 29.4 vs 30.2 us, bank 128 x 1e5: 4.3e10 vs 5.0e10 particle-steps/s.
    // LLPF_SCHEDULE=merged pins the first, any other value the second.
    // (round 6: below threshold 1 the split schedule stores no quanta and moves 16 bytes per lane on the steps that do not resample — it
    //  overtakes the merged one from ~1.3 M particles on: N = 1.5e6 / 2e6 / 3e6 at threshold 0.1 27.9 / 34.4 / 43.9 against 29.6 / 36.0 / 48.3 us;
    //  at threshold 1.0 the two stay within 4 % of each other up to 3 M, profiles/r06_schedule_crossover_ab.txt)
    const int64_t merged_max = (f.thr < 1.0) ? ((int64_t)5 << 18) : ((int64_t)3 << 20);
    p.merged = f.hist || (s.schedule >= 0 ? s.schedule != 0 : FNs <= merged_max);
    // a likelihood of the model's own that declares no bound (loglik without loglik_bound): there is nothing to normalise against ahead
    // of the weights, so every timestep takes the exact-max form — as launches of the run loop (k_norm in exact form in front of the
    // head), not as a failed bound test that the host notices and redoes (one round trip per timestep until round 4)
    p.no_bound = user_model && f.traits > 0 && (f.traits & LLPF_TRAIT_LOGLIK) && !(f.traits & LLPF_TRAIT_LOGLIK_BOUND);
    // (a model without a bound: the weighting launches form no sums at all — a step without a measurement would otherwise leave real ones
    // in the slot, against the finite bound max(w), and the exact-form k_norm in front of the next head would add to them)
    p.acc_in_weighting = p.merged && !p.no_bound;
    // Split schedule in front of the fused kernel, thresholds below 1: k_norm stores NO quanta (launch_norm, bound bit 1) and the fused
    // kernel's scan forms its tile's quanta from the weights (ResArgs::lazy_q) — a step that does not resample moves 16 bytes per
    // particle less (the 8 k_norm stored, the 8 the fused kernel requested before it knew), one that does the same bytes plus an exp per
    // source, which is why a filter that resamples at every step keeps the stored form.  The scan then reads weights that other blocks
    // of the same launch are replacing with the next ones: such a run alternates between two weight buffers (BankDev::w / w_next; the
    // second is allocated by the first such run and starts as a copy, so that its padding holds -Inf too).  LLPF_LAZY_Q=0: stored form.
    p.lazy_run = !p.merged && !p.unfused && !p.no_bound && f.thr < 1.0 && s.lazy_q != 0;
    // Merged fused run at threshold 1: every step resamples, so the weights a launch forms are never read again — the next step's prior is
    // log(1/N), its head consumes their integer sums and quanta, and the run ends uniform (k_post_predict) — and the fused launches do not
    // store them (k_resprop<..., RUN_SKIP_W>: 8 of the 44 bytes an output writes).  Their one reader is the exact redo of a failed bound test, in
    // front of which the weights of the flagged filters are formed again (host/run.hpp: reweight_flagged).  Not for one-tile filters (their
    // kernel redoes a failed test in place, from the stored weights) nor for the Rao-Blackwellized model (its weighting also updates the
    // linear substate).  LLPF_SKIP_W=0: the storing form.
    const bool skip_w = !p.unfused && p.acc_in_weighting && !rbm && f.thr == 1.0 && f.P2 > 1 && s.skip_w != 0;
    // ... nor the ancestors of the outputs with an owner (k_resprop<..., RUN_SKIP_ANC>: 4 more bytes, one more store).  Every launch of such a
    // run rewrites all N entries, so only those of the run's last launch — which has no weighting phase and keeps storing — reach the accessor,
    // the "stale j" rule of later verbs or k_resample; inside the run the one reader is the next launch's rounds of [c_end, M), for which
    // the entry of output M - 1 is kept current (kernels/resprop.hpp).  LLPF_SKIP_ANC=0: every launch stores its ancestors.
    const bool skip_anc = skip_w && s.skip_anc != 0;
    // nontemporal accesses on the steps that do not resample: working sets well beyond the Infinity Cache (LLPF_NT_ID=0|1 pins it)
    p.nt_id = s.nt_id >= 0 ? s.nt_id : (FNs >= ((int64_t)7 << 20) ? 1 : 0);
    // weighted means come out of the normalise / weighting kernels (partial sums over the nx rows they read anyway); the
    // model with per-particle covariance takes them from a k_wmean launch per step over its [xn; xl] rows instead
    p.want_xm = f.xmean && !rbfull;
    p.xm_launch = f.xmean && rbfull;
    // ... and what else such a run knows before its first launch: it resamples systematically and wants no weighted means — the launches
    // that store no ancestors are then k_resprop<..., RUN_LEAN>, which holds neither the stratified counts (a Philox block per threshold) nor
    // the means and tests neither (the same bits).  The kernel exists for the linear-Gaussian model with one or two states; every other
    // shape keeps the level below.  LLPF_LEAN=0: the kernel with the run-time tests.
    const bool lean = skip_anc && f.strategy == LLPF_RESAMPLE_SYSTEMATIC && !p.want_xm && f.model_id == LLPF_MODEL_LINEAR_GAUSSIAN && f.nx <= 2 && s.lean != 0;
    p.level = lean ? RUN_LEAN : skip_anc ? RUN_SKIP_ANC : skip_w ? RUN_SKIP_W : RUN_STORES;
    // ... and that the maximum a level-3 launch leaves is read by nobody when the launch behind it is a level-3 launch too: that head takes
    // the bound for its offset, tests the integer sums and the NaN count, and publishes the maximum in two scalars that the head after it
    // overwrites unread (DESIGN.md §4 goes through every reader).  Such launches are RUN_NO_MAX (launch_level below).  LLPF_SKIP_MAX=0: none is.
    p.skip_max = (LLPF_SKIP_MAX && lean && s.skip_max != 0) ? 1 : 0;
    // The run ends in the buffer it began in (a handle's weights do not move between runs: one captured graph per shape, not two that
    // alternate): T - 1 steps have a weighting phase; when that number is odd, step 0 keeps the stored form and weights in place.
    p.k_pp0 = (p.lazy_run && ((f.T - 1) & 1)) ? 1 : 0;
    p.ablate = s.ablate;
    p.ll_steps = f.ll_steps; p.multi = f.multi; p.xcov = f.xcov; p.xquant = f.xquant;
    // a captured graph holds no host round trip: not with history (row copies, or staging that is freed), not while events are collected
    p.use_graph = !f.hist && !f.profiling && !s.debug_timing && s.graph != 0;
    return p;
}
// The level of one fused launch of the run: the exact redo of a failed bound test (`fast` false) reads stored weights and keeps the
// storing form; the run's last launch (`weight` false: no weighting phase) forms no weights and leaves the ancestors the run ends with.
static inline int launch_level(const RunForm& p, bool fast, bool weight) {
    return !fast ? RUN_STORES : !weight ? std::min<int>(p.level, RUN_SKIP_W) : p.level;
}
// ... with what the plan decided besides.  `next_weight`: the launch behind this one has a weighting phase as well (step k + 2 < T), so it
// is a level-3 or level-4 launch whose head reads no maximum — unless that head's bound test fails, and then the exact redo forms the
// weights again by the weighting launch (RunLoop::reweight_flagged), which leaves its own maximum in the slot.  The run's last weighting
// launch keeps level 3: the general head of the run's last launch combines its maximum, and what that head publishes is what the run
// leaves (k_post_predict resets it only when the step resampled).  The first launch behind an exact redo may be RUN_NO_MAX like any other.
static inline int launch_level(const RunKey& p, bool fast, bool weight, bool next_weight) {
    const int level = launch_level(static_cast<const RunForm&>(p), fast, weight);
    return (level == RUN_LEAN && p.skip_max && next_weight) ? RUN_NO_MAX : level;
}
// The step of the systematic thresholds, 1 / M, as a level-3 launch gets it from the host (ResArgs::inv_M) instead of dividing in every
// wave.  IEEE division is correctly rounded on the host and on the device, so this is the double the kernel's own 1.0 / (double)M is:
// the same bits (tests/test_lean_inv_m.py holds it against the oracle's expression).
static inline double lean_inv_M(int32_t M) { return 1.0 / (double)M; }

// ---- the host-side state of a run's timesteps (the device may have to be re-driven from a step whose bound test failed) ----
struct RunEntry { int cur, qcur, parity; uint32_t n_predict; int64_t t_index; int nslot; };      // Bank's state when the run began; nslot = ACC_NSLOT
struct StepState {
    int cur, qcur;
    int parity;              // slot the next weighting writes
    uint32_t n_predict;
    int64_t t_index;
    int wbuf;                // which of the run's two weight buffers holds the current weights (0: the one it began in)
    bool w_pingpong;         // the fused kernel writes the weights it forms to the other buffer
};
// the first weighting runs in the state at entry, in place
static inline StepState entry_state(const RunEntry& e) { return StepState{e.cur, e.qcur, e.parity, e.n_predict, e.t_index, 0, false}; }
// state in which step k's head runs (initial weighting done, k steps done)
static inline StepState step_state(const RunEntry& e, const RunForm& p, int64_t T, int64_t k) {
    StepState s;
    s.cur = e.cur ^ (int)(k & 1);
    s.qcur = e.qcur ^ 1 ^ (int)(k & 1);
    s.parity = (e.parity + 1 + (int)(k % e.nslot)) % e.nslot;      // slot the weighting of step k writes
    s.n_predict = e.n_predict + (uint32_t)k;
    s.t_index = e.t_index + k;
    // weights in front of step k: every step before it had a weighting phase that wrote the other buffer (the run's last step has none)
    const int64_t wsw = std::max<int64_t>(0, std::min<int64_t>(k, T - 1 > 0 ? T - 1 : 0) - p.k_pp0);
    s.wbuf = (p.lazy_run && (wsw & 1)) ? 1 : 0;
    s.w_pingpong = p.lazy_run && k >= p.k_pp0;
    return s;
}
// slot the head of step k consumes: the one the weighting of step k - 1 (or the first weighting) wrote
static inline int head_slot(const RunEntry& e, int64_t k) { return (e.parity + (int)(k % e.nslot)) % e.nslot; }
// state the run leaves: T steps done, back in the buffer it began in, weighting in place
static inline StepState end_state(const RunEntry& e, const RunForm& p, int64_t T) {
    StepState s = step_state(e, p, T, T);
    s.w_pingpong = false;
    s.qcur = e.qcur ^ (int)(T & 1);                                // the last step has no weighting phase: no quanta swap
    s.parity = (e.parity + (int)(T % e.nslot)) % e.nslot;
    return s;
}
