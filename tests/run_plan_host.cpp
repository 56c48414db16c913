// run_plan_host.cpp — the form of a run (csrc/host/run_plan.hpp: make_run_plan, launch_level, step_state, RunForm) checked without a
// device (tests/test_run_plan.py).  The header makes no HIP call, so a host compiler alone builds this program; it links nothing.
// The expected values are the rules of the run loop written out by hand (the thresholds 5<<18, 3<<20 and 7<<20 particles, the
// hysteresis 5 % / 8 %, ...), never the output of the code under test.
// Build: c++ -std=c++17 -fsanitize=address,undefined run_plan_host.cpp -o run_plan_host
// Prints one line per check, in two sections (# form, # level); the exit status is the number of failed checks.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../lowlevelparticlefilters.jl_amd/csrc/host/run_plan.hpp"

static int failed = 0;
static void check(bool ok, const std::string& what) {
    printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++failed;
}
#define CHECK(cond) check((cond), std::string(name) + ": " #cond)

static const int64_t TILE = 1024;      // Ns is N rounded up to whole tiles
static const int NSLOT = 3;            // ACC_NSLOT (csrc/engine.hpp)

// linear-Gaussian, nx = 2, one filter of FNs particles in more than one tile, no output asked for, a handle's first run
static RunFacts lg(int64_t FNs, double thr) {
    RunFacts f;
    f.model_id = LLPF_MODEL_LINEAR_GAUSSIAN; f.nx = 2; f.F = 1; f.Ns = FNs; f.P2 = 8;
    f.strategy = LLPF_RESAMPLE_SYSTEMATIC; f.thr = thr; f.T = 10;
    return f;
}

static void plan_cases() {
    const int64_t M = (int64_t)1 << 20;
    const char* name;
    {
        name = "1M thr 1";
        const RunPlan p = make_run_plan(lg(M, 1.0));
        CHECK(!p.unfused && p.merged && p.acc_in_weighting && p.level >= 1 && !p.lazy_run && p.nt_id == 0 && p.use_graph);
        CHECK(!p.no_bound && !p.fx_capable && !p.source_fx && !p.want_xm && !p.xm_launch && p.k_pp0 == 0 && p.ablate == 0);
    }
    {
        name = "1M thr 0.1";
        const RunPlan p = make_run_plan(lg(M, 0.1));
        CHECK(!p.unfused && p.merged && !p.lazy_run && p.level == 0);
    }
    {
        name = "2M thr 0.1";
        RunFacts f = lg(2 * M, 0.1);
        const RunPlan p = make_run_plan(f);
        CHECK(!p.unfused && !p.merged && !p.acc_in_weighting && p.lazy_run && p.level == 0);
        CHECK(p.k_pp0 == 1);                          // T = 10: nine weighting phases
        f.T = 11;
        CHECK(make_run_plan(f).k_pp0 == 0);
    }
    {
        name = "4M thr 1";
        const RunPlan p = make_run_plan(lg(4 * M, 1.0));
        CHECK(!p.unfused && !p.merged && !p.lazy_run && p.level == 0 && p.nt_id == 0);
    }
    {
        name = "16M thr 0.1";
        const RunPlan p = make_run_plan(lg(16 * M, 0.1));
        CHECK(!p.unfused && !p.merged && p.lazy_run && p.nt_id == 1);
    }
    {
        name = "thresholds";
        CHECK(make_run_plan(lg((int64_t)5 << 18, 0.1)).merged && !make_run_plan(lg((int64_t)5 << 18, 0.1)).lazy_run);
        CHECK(!make_run_plan(lg(((int64_t)5 << 18) + TILE, 0.1)).merged && make_run_plan(lg(((int64_t)5 << 18) + TILE, 0.1)).lazy_run);
        CHECK(make_run_plan(lg(((int64_t)5 << 18) + TILE, 1.0)).merged);      // the lower limit is the one of thresholds below 1
        CHECK(make_run_plan(lg((int64_t)3 << 20, 1.0)).merged && make_run_plan(lg((int64_t)3 << 20, 1.0)).level >= 1);
        CHECK(!make_run_plan(lg(((int64_t)3 << 20) + TILE, 1.0)).merged && make_run_plan(lg(((int64_t)3 << 20) + TILE, 1.0)).level == 0);
        CHECK(make_run_plan(lg(((int64_t)7 << 20) - TILE, 1.0)).nt_id == 0);
        CHECK(make_run_plan(lg((int64_t)7 << 20, 1.0)).nt_id == 1);
        CHECK(make_run_plan(lg(((int64_t)7 << 20) + TILE, 1.0)).nt_id == 1);
        RunFacts bank = lg(TILE, 1.0);                // the limits count the particles of the whole bank
        bank.F = 3 << 10;
        CHECK(make_run_plan(bank).merged);
        bank.F += 1;
        CHECK(!make_run_plan(bank).merged);
    }
    {
        name = "quad-tank";
        RunFacts f = lg(M, 0.5);
        f.model_id = LLPF_MODEL_QUADTANK_RK4; f.nx = 4; f.fx_supported = true;
        RunPlan p = make_run_plan(f);                 // surv_frac = -1: a first run
        CHECK(p.unfused && p.fx_capable && p.source_fx && p.use_fx && p.merged && p.level == 0 && !p.lazy_run);
        // the hysteresis: below 5 % source-side, above 8 % per output, in between what it was
        for (int from = 0; from < 2; ++from) {
            f.use_fx = from != 0;
            f.surv_frac = 0.04; p = make_run_plan(f);
            CHECK(p.use_fx && p.source_fx);
            f.surv_frac = 0.06; p = make_run_plan(f);
            CHECK(p.use_fx == (from != 0) && p.source_fx == from);
            f.surv_frac = 0.09; p = make_run_plan(f);
            CHECK(!p.use_fx && !p.source_fx && p.fx_capable);
        }
        f.use_fx = false; f.surv_frac = 0.5; f.sw.source_fx = 1; p = make_run_plan(f);
        CHECK(p.source_fx && !p.use_fx);              // LLPF_SOURCE_FX=1 pins the run's form; the handle's own choice goes on
        f.use_fx = true; f.surv_frac = 0.01; f.sw.source_fx = 0; p = make_run_plan(f);
        CHECK(!p.source_fx && p.use_fx && p.fx_capable);
        f.sw.source_fx = -1; f.fx_supported = false; p = make_run_plan(f);
        CHECK(p.unfused && !p.fx_capable && !p.source_fx);
        f.fx_supported = true; f.sw.unfused = 0; p = make_run_plan(f);
        CHECK(!p.unfused && !p.fx_capable && !p.source_fx);      // the fused form has no source-side dynamics
    }
    {
        name = "nx 3";
        RunFacts f = lg(M, 1.0);
        f.nx = 3;
        CHECK(make_run_plan(f).unfused && make_run_plan(f).level == 0);
        f.sw.unfused = 0;
        CHECK(!make_run_plan(f).unfused && make_run_plan(f).level >= 1);
        f.nx = 2; f.sw.unfused = 1;
        CHECK(make_run_plan(f).unfused);
    }
    {
        name = "residual";
        RunFacts f = lg(M, 1.0);
        f.strategy = LLPF_RESAMPLE_RESIDUAL;
        CHECK(make_run_plan(f).unfused);
        f.sw.unfused = 0;
        CHECK(make_run_plan(f).unfused);              // not a matter of speed: the switch does not reach it
    }
    {
        name = "user model";
        RunFacts f = lg(M, 1.0);
        f.model_id = LLPF_MODEL_USER_BASE + 3; f.traits = LLPF_TRAIT_LOGLIK;
        RunPlan p = make_run_plan(f);
        CHECK(p.unfused && p.no_bound && p.merged && !p.acc_in_weighting && p.level == 0 && !p.lazy_run);
        f.traits = LLPF_TRAIT_LOGLIK | LLPF_TRAIT_LOGLIK_BOUND; p = make_run_plan(f);
        CHECK(p.unfused && !p.no_bound && p.acc_in_weighting);
        f.traits = LLPF_TRAIT_NOISE; p = make_run_plan(f);
        CHECK(p.unfused && !p.no_bound);
        f.traits = -1; p = make_run_plan(f);          // an id nobody compiled
        CHECK(p.unfused && !p.no_bound);
        f.model_id = LLPF_MODEL_LINEAR_GAUSSIAN; f.traits = LLPF_TRAIT_LOGLIK; p = make_run_plan(f);
        CHECK(!p.unfused && !p.no_bound);             // the traits are those of a run-time compiled model
    }
    {
        name = "outputs";
        RunFacts f = lg(16 * M, 0.1);
        f.hist = true;
        RunPlan p = make_run_plan(f);
        CHECK(p.unfused && p.merged && !p.lazy_run && !p.use_graph);
        f.sw.schedule = 0;
        CHECK(make_run_plan(f).merged);               // history is copied out of the merged schedule whatever LLPF_SCHEDULE says
        f = lg(M, 1.0); f.xcov = true; p = make_run_plan(f);
        CHECK(p.unfused && p.use_graph && p.xcov && !p.xquant && p.level == 0);
        f = lg(M, 1.0); f.xquant = true; p = make_run_plan(f);
        CHECK(p.unfused && p.use_graph && p.xquant && !p.xcov);
        f = lg(M, 1.0); f.xmean = true; f.ll_steps = true; f.multi = true; p = make_run_plan(f);
        CHECK(!p.unfused && p.want_xm && !p.xm_launch && p.ll_steps && p.multi && p.level >= 1);
        f.model_id = LLPF_MODEL_RB_BILINEAR; p = make_run_plan(f);
        CHECK(p.unfused && !p.want_xm && p.xm_launch);
    }
    {
        name = "no skip_w";
        RunFacts f = lg(M, 1.0);
        f.P2 = 1;
        CHECK(make_run_plan(f).level == 0 && !make_run_plan(f).unfused);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_RB_LINEAR;
        CHECK(make_run_plan(f).level == 0 && !make_run_plan(f).unfused && make_run_plan(f).acc_in_weighting);
    }
    {
        name = "no graph";
        RunFacts f = lg(M, 1.0);
        f.profiling = true;
        CHECK(!make_run_plan(f).use_graph);
        f = lg(M, 1.0); f.sw.graph = 0;
        CHECK(!make_run_plan(f).use_graph);
        f.sw.graph = 1;
        CHECK(make_run_plan(f).use_graph);
        f = lg(M, 1.0); f.sw.debug_timing = true;
        CHECK(!make_run_plan(f).use_graph);
    }
    {
        name = "switches";
        RunFacts f = lg(16 * M, 0.1);
        f.sw.schedule = 1;
        CHECK(make_run_plan(f).merged && !make_run_plan(f).lazy_run);
        f = lg(M, 1.0); f.sw.schedule = 0;
        CHECK(!make_run_plan(f).merged && make_run_plan(f).level == 0 && !make_run_plan(f).lazy_run);
        f = lg(2 * M, 0.1); f.sw.lazy_q = 0;
        CHECK(!make_run_plan(f).merged && !make_run_plan(f).lazy_run && make_run_plan(f).k_pp0 == 0);
        f.sw.lazy_q = 1;
        CHECK(make_run_plan(f).lazy_run);
        f = lg(M, 1.0); f.sw.skip_w = 0;
        CHECK(make_run_plan(f).merged && make_run_plan(f).level == 0);
        f.sw.skip_w = 1;
        CHECK(make_run_plan(f).level >= 1);
        f = lg(16 * M, 0.1); f.sw.nt_id = 0;
        CHECK(make_run_plan(f).nt_id == 0);
        f = lg(M, 1.0); f.sw.nt_id = 1;
        CHECK(make_run_plan(f).nt_id == 1);
        f = lg(M, 1.0); f.sw.ablate = 0x12345;
        CHECK(make_run_plan(f).ablate == 0x12345);
    }
    {
        name = "environment";
        RunSwitches s = read_run_switches();
        CHECK(s.unfused == -1 && s.source_fx == -1 && s.schedule == -1 && s.nt_id == -1 && s.lazy_q == -1 && s.skip_w == -1 && s.graph == -1 && s.ablate == 0 && !s.debug_timing);
        setenv("LLPF_SCHEDULE", "merged", 1); setenv("LLPF_UNFUSED", "0", 1); setenv("LLPF_SOURCE_FX", "1", 1);
        setenv("LLPF_NT_ID", "0", 1); setenv("LLPF_LAZY_Q", "0", 1); setenv("LLPF_SKIP_W", "0", 1);
        setenv("LLPF_GRAPH", "0", 1);
        s = read_run_switches();
        CHECK(s.schedule == 1 && s.unfused == 0 && s.source_fx == 1 && s.nt_id == 0 && s.lazy_q == 0 && s.skip_w == 0);
        CHECK(s.graph == -1);                         // read once per process
        setenv("LLPF_SCHEDULE", "split", 1);
        CHECK(read_run_switches().schedule == 0);
        setenv("LLPF_SCHEDULE", "anything", 1);
        CHECK(read_run_switches().schedule == 0);
        unsetenv("LLPF_SCHEDULE"); unsetenv("LLPF_UNFUSED");
        CHECK(read_run_switches().schedule == -1 && read_run_switches().unfused == -1);
        for (const char* v : {"LLPF_SOURCE_FX", "LLPF_NT_ID", "LLPF_LAZY_Q", "LLPF_SKIP_W", "LLPF_GRAPH"}) unsetenv(v);
    }
}

// The host-side state of the timesteps of a run of T steps, from every state a run can begin in.
static void step_cases() {
    for (int T = 1; T <= 9; ++T)
        for (int lazy = 0; lazy < 2; ++lazy) {
            RunForm p{};
            p.lazy_run = lazy;
            p.k_pp0 = (lazy && ((T - 1) & 1)) ? 1 : 0;      // an odd number of weighting phases: step 0 weights in place
            bool home = true, pingpong = true, slots = true, counters = true, planes = true, buffers = true;
            for (int par0 = 0; par0 < NSLOT; ++par0)
                for (int cur0 = 0; cur0 < 2; ++cur0)
                    for (int qcur0 = 0; qcur0 < 2; ++qcur0) {
                        const RunEntry e{cur0, qcur0, par0, 1000u + (uint32_t)par0, 70 + cur0, NSLOT};
                        const StepState s0 = entry_state(e);
                        planes = planes && s0.cur == cur0 && s0.qcur == qcur0 && s0.parity == par0 && s0.wbuf == 0 && !s0.w_pingpong;
                        int written = par0;                 // the slot the last weighting wrote: the first weighting's
                        for (int k = 0; k <= T; ++k) {
                            const StepState s = step_state(e, p, T, k);
                            pingpong = pingpong && s.w_pingpong == (lazy && k >= p.k_pp0);
                            slots = slots && head_slot(e, k) == written && s.parity == (written + 1) % NSLOT;
                            written = s.parity;
                            counters = counters && s.n_predict == e.n_predict + (uint32_t)k && s.t_index == e.t_index + k;
                            // each step swaps the particle planes, each weighting (the first one included) the quanta buffers
                            planes = planes && s.cur == (cur0 ^ (k & 1)) && s.qcur == (qcur0 ^ 1 ^ (k & 1));
                            // a step that weights (all but the last) into the other buffer moves the weights there; no other one does
                            if (k < T) {
                                const bool moves = s.w_pingpong && k + 1 < T;
                                buffers = buffers && step_state(e, p, T, k + 1).wbuf == (s.wbuf ^ (moves ? 1 : 0));
                            }
                            if (!lazy) buffers = buffers && s.wbuf == 0;
                        }
                        const StepState end = end_state(e, p, T);
                        home = home && step_state(e, p, T, 0).wbuf == 0 && step_state(e, p, T, T).wbuf == 0 && end.wbuf == 0 && !end.w_pingpong;
                        // T steps, T weightings (the first one and T - 1 in the steps): the last step has no weighting phase
                        planes = planes && end.cur == (cur0 ^ (T & 1)) && end.qcur == (qcur0 ^ (T & 1));
                        slots = slots && end.parity == (par0 + T) % NSLOT;
                        counters = counters && end.n_predict == e.n_predict + (uint32_t)T && end.t_index == e.t_index + T;
                    }
            const std::string name = "T " + std::to_string(T) + (lazy ? " lazy" : " stored");
            check(home, name + ": the run ends in the weight buffer it began in");
            check(pingpong, name + ": w_pingpong is off before k_pp0 and on from it");
            check(slots, name + ": the head of step k reads the slot the weighting before it wrote");
            check(counters, name + ": n_predict and t_index advance by k");
            check(planes, name + ": particle planes and quanta buffers alternate");
            check(buffers, name + ": the weights move only with a step that weights into the other buffer");
        }
}

// The key of a captured graph holds a RunForm: two that differ in any one field are different keys.
static void key_cases() {
    const char* name = "graph key";
    RunFacts f = lg((int64_t)1 << 20, 1.0);
    const RunForm a = make_run_plan(f);
    RunForm same = a;
    CHECK(a == same);
    const size_t n = sizeof(RunForm) / sizeof(int);
    CHECK(n == 17);                                   // the fields of RunForm, all of them ints
    size_t differ = 0;
    for (size_t i = 0; i < n; ++i) {
        RunForm c = a;
        reinterpret_cast<int*>(&c)[i] ^= 1;
        differ += (c == a) ? 0 : 1;
    }
    CHECK(differ == n);
    RunForm c = a;
    c.ablate = 1 << 21;                               // (a bit that once aliased a schedule bit of a packed key)
    CHECK(!(c == a));
    f.sw.nt_id = 1;
    CHECK(!(make_run_plan(f) == a));
    f = lg((int64_t)1 << 20, 1.0); f.surv_frac = 0.5; f.use_fx = false;
    CHECK(make_run_plan(f) == a);                     // what the handle will do next is no part of this run's form
    // plans that differ in one of the three switches of the level are different keys, and differ in the level alone
    CHECK(sizeof(RunForm) == 17 * sizeof(int));
    for (int which = 0; which < 3; ++which) {
        f = lg((int64_t)1 << 20, 1.0);
        (which == 0 ? f.sw.skip_w : which == 1 ? f.sw.skip_anc : f.sw.lean) = 0;
        const RunForm b = make_run_plan(f);
        CHECK(!(a == b) && a.level == 3 && b.level == which);
        c = b; c.level = a.level;
        CHECK(c == a);
        c = a; c.level = b.level;
        CHECK(c == b && !(c == a));
    }
}

// The level of a run at resample_threshold 1 (RunForm::level): 0 where the precondition fails — fused, merged schedule with sums in the
// weighting, not Rao-Blackwellized, threshold exactly 1, more than one tile — else the highest level the facts and the switches allow.
static void level_cases() {
    const int64_t M = (int64_t)1 << 20;
    const char* name = "levels";
    CHECK(RUN_STORES == 0 && RUN_SKIP_W == 1 && RUN_SKIP_ANC == 2 && RUN_LEAN == 3);
    name = "preconditions";
    CHECK(make_run_plan(lg(M, 1.0)).level == 3);                                 // the headline workload
    CHECK(make_run_plan(lg(M, 0.1)).level == 0);
    CHECK(make_run_plan(lg(M, 0.5)).level == 0);
    CHECK(make_run_plan(lg(M, 0.999999)).level == 0);
    CHECK(make_run_plan(lg((int64_t)3 << 20, 1.0)).level >= 2);
    CHECK(make_run_plan(lg(((int64_t)3 << 20) + TILE, 1.0)).level == 0);         // the split schedule
    {
        RunFacts f = lg(M, 1.0); f.P2 = 1;
        CHECK(make_run_plan(f).level == 0);                                      // one tile
        f.P2 = 2;
        CHECK(make_run_plan(f).level >= 2);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_RB_LINEAR;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_QUADTANK_RK4; f.nx = 4;
        CHECK(make_run_plan(f).level == 0);                                      // the balanced form
        f.sw.unfused = 0;
        CHECK(!make_run_plan(f).unfused && make_run_plan(f).level == 2);         // fused by the switch: the lean kernel does not exist for it
        f = lg(M, 1.0); f.nx = 3;
        CHECK(make_run_plan(f).level == 0);
        f.sw.unfused = 0;
        CHECK(!make_run_plan(f).unfused && make_run_plan(f).level == 2);         // ... nor for three states
        f = lg(M, 1.0); f.nx = 1;
        CHECK(make_run_plan(f).level == 3);
        f = lg(M, 1.0); f.strategy = LLPF_RESAMPLE_RESIDUAL;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.strategy = LLPF_RESAMPLE_STRATIFIED;
        CHECK(make_run_plan(f).level == 2);
        f = lg(M, 1.0); f.hist = true;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.xcov = true;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.xquant = true;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.xmean = true;
        CHECK(make_run_plan(f).want_xm && make_run_plan(f).level == 2);
        f.ll_steps = true; f.multi = true;
        CHECK(make_run_plan(f).level == 2);
        f = lg(M, 1.0); f.ll_steps = true; f.multi = true;
        CHECK(make_run_plan(f).level == 3);                                      // outputs that are not means do not matter
        f = lg(M, 1.0); f.sw.schedule = 0;
        CHECK(make_run_plan(f).level == 0);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_USER_BASE + 3; f.traits = LLPF_TRAIT_LOGLIK;
        CHECK(make_run_plan(f).level == 0);
        f = lg(TILE, 1.0); f.F = 3 << 10;                                        // a bank in the merged schedule
        CHECK(make_run_plan(f).merged && make_run_plan(f).level == 3);
    }
    name = "switches";
    {
        RunFacts f = lg(M, 1.0);
        f.sw.lean = 0;
        CHECK(make_run_plan(f).level == 2);                                      // the same run, the kernel with the tests
        f.sw.lean = 1;
        CHECK(make_run_plan(f).level == 3);
        f.sw.skip_anc = 0;
        CHECK(make_run_plan(f).level == 1);                                      // the ancestor-storing form of the same run
        f.sw.skip_anc = 1;
        CHECK(make_run_plan(f).level == 3);
        f.sw.skip_w = 0;
        CHECK(make_run_plan(f).level == 0);                                      // nothing is left out where the weights are stored
        f = lg(M, 0.1); f.sw.skip_anc = 1; f.sw.lean = 1;
        CHECK(make_run_plan(f).level == 0);                                      // a switch pins a lower level; it cannot force a higher one
        f = lg(M, 0.5); f.sw.lean = 1;
        CHECK(make_run_plan(f).level == 0);
        // every shape: level >= 1 is the precondition and LLPF_SKIP_W, level >= 2 that and LLPF_SKIP_ANC
        bool follows = true;
        int shapes = 0;
        for (int thr1 = 0; thr1 < 2; ++thr1)
            for (int P2 = 1; P2 <= 2; ++P2)
                for (int rb = 0; rb < 2; ++rb)
                    for (int unf = -1; unf <= 1; ++unf)
                        for (int sch = -1; sch <= 1; ++sch)
                            for (int sw = -1; sw <= 1; ++sw)
                                for (int sa = -1; sa <= 1; ++sa, ++shapes) {
                                    RunFacts g = lg(M, thr1 ? 1.0 : 0.5);
                                    g.P2 = P2; g.model_id = rb ? LLPF_MODEL_RB_LINEAR : LLPF_MODEL_LINEAR_GAUSSIAN;
                                    g.sw.unfused = unf; g.sw.schedule = sch; g.sw.skip_w = sw; g.sw.skip_anc = sa;
                                    const RunPlan p = make_run_plan(g);
                                    const bool fused = unf != 1, merged = sch != 0;
                                    const bool w = fused && merged && !rb && thr1 && P2 > 1 && sw != 0;
                                    follows = follows && (p.level >= 1) == w && (p.level >= 2) == (w && sa != 0);
                                }
        check(follows && shapes == 648, "switches: level >= 2 == level 1's preconditions && LLPF_SKIP_ANC != 0, over 648 shapes");
        // every shape: level 3 where the run stores no ancestors, resamples systematically, wants no means, is LinGauss<NX <= 2> and LLPF_LEAN != 0
        follows = true; shapes = 0;
        const int strategies[3] = {LLPF_RESAMPLE_SYSTEMATIC, LLPF_RESAMPLE_STRATIFIED, LLPF_RESAMPLE_RESIDUAL};
        const int models[3] = {LLPF_MODEL_LINEAR_GAUSSIAN, LLPF_MODEL_RB_LINEAR, LLPF_MODEL_QUADTANK_RK4};
        for (int si = 0; si < 3; ++si)
            for (int xm = 0; xm < 2; ++xm)
                for (int thr1 = 0; thr1 < 2; ++thr1)
                    for (int P2 = 1; P2 <= 2; ++P2)
                        for (int mi = 0; mi < 3; ++mi)
                            for (int sa = -1; sa <= 1; ++sa)
                                for (int ln = -1; ln <= 1; ++ln, ++shapes) {
                                    RunFacts g = lg(M, thr1 ? 1.0 : 0.5);
                                    g.strategy = strategies[si]; g.xmean = xm != 0; g.P2 = P2; g.model_id = models[mi];
                                    g.nx = models[mi] == LLPF_MODEL_QUADTANK_RK4 ? 4 : 2;
                                    g.sw.skip_anc = sa; g.sw.lean = ln;
                                    const RunPlan p = make_run_plan(g);
                                    const bool fused = models[mi] != LLPF_MODEL_QUADTANK_RK4 && strategies[si] != LLPF_RESAMPLE_RESIDUAL;
                                    const bool w = fused && models[mi] == LLPF_MODEL_LINEAR_GAUSSIAN && thr1 && P2 > 1;
                                    const bool lean = w && sa != 0 && strategies[si] == LLPF_RESAMPLE_SYSTEMATIC && !xm && ln != 0 &&
                                                      models[mi] == LLPF_MODEL_LINEAR_GAUSSIAN && g.nx <= 2;
                                    follows = follows && p.level == (lean ? 3 : (w && sa != 0) ? 2 : w ? 1 : 0);
                                }
        check(follows && shapes == 648, "switches: level 3 == level 2 && systematic && !xmean && LinGauss<NX <= 2> && LLPF_LEAN != 0, over 648 shapes");
        // the 27 settings of the three switches on the headline workload: the level by hand, and clearing a switch never raises it
        bool by_hand = true, monotone = true;
        for (int sw = -1; sw <= 1; ++sw)
            for (int sa = -1; sa <= 1; ++sa)
                for (int ln = -1; ln <= 1; ++ln) {
                    RunFacts g = lg(M, 1.0);
                    g.sw.skip_w = sw; g.sw.skip_anc = sa; g.sw.lean = ln;
                    const int level = make_run_plan(g).level;
                    by_hand = by_hand && level == (sw == 0 ? 0 : sa == 0 ? 1 : ln == 0 ? 2 : 3);
                    for (int which = 0; which < 3; ++which) {
                        RunFacts h = g;
                        (which == 0 ? h.sw.skip_w : which == 1 ? h.sw.skip_anc : h.sw.lean) = 0;
                        monotone = monotone && make_run_plan(h).level <= level;
                    }
                }
        check(by_hand, "switches: LLPF_SKIP_W=0 caps the level at 0, LLPF_SKIP_ANC=0 at 1, LLPF_LEAN=0 at 2, over 27 settings");
        check(monotone, "switches: clearing a switch never raises the level, over 27 settings");
    }
    name = "environment";
    {
        CHECK(read_run_switches().skip_anc == -1 && read_run_switches().lean == -1);
        setenv("LLPF_SKIP_ANC", "0", 1);
        CHECK(read_run_switches().skip_anc == 0);
        RunFacts f = lg(M, 1.0);
        f.sw = read_run_switches();
        CHECK(make_run_plan(f).level == 1);
        setenv("LLPF_SKIP_ANC", "1", 1);
        CHECK(read_run_switches().skip_anc == 1);
        unsetenv("LLPF_SKIP_ANC");
        CHECK(read_run_switches().skip_anc == -1);
        setenv("LLPF_LEAN", "0", 1);
        CHECK(read_run_switches().lean == 0);
        f.sw = read_run_switches();
        CHECK(make_run_plan(f).level == 2);
        setenv("LLPF_LEAN", "1", 1);
        CHECK(read_run_switches().lean == 1);
        unsetenv("LLPF_LEAN");
        CHECK(read_run_switches().lean == -1);
    }
    // the level of one launch: 0 for the exact redo, at most 1 for the run's last launch, the plan's otherwise
    name = "launch_level";
    {
        const int want[4][2][2] = {      // [level][fast][weight]
            {{0, 0}, {0, 0}},
            {{0, 0}, {1, 1}},
            {{0, 0}, {1, 2}},
            {{0, 0}, {1, 3}},
        };
        bool ok = true;
        for (int level = 0; level < 4; ++level)
            for (int fast = 0; fast < 2; ++fast)
                for (int weight = 0; weight < 2; ++weight) {
                    RunForm p{};
                    p.level = level;
                    ok = ok && launch_level(p, fast != 0, weight != 0) == want[level][fast][weight];
                }
        check(ok, "launch_level: every (level, fast, weight)");
    }
    // the host-side state of every timestep is the same at every level
    {
        bool same = true;
        for (int T = 1; T <= 9; ++T)
            for (int par0 = 0; par0 < NSLOT; ++par0)
                for (int cur0 = 0; cur0 < 2; ++cur0)
                    for (int qcur0 = 0; qcur0 < 2; ++qcur0)
                        for (int level = 1; level < 4; ++level) {
                            const RunEntry e{cur0, qcur0, par0, 1000u + (uint32_t)par0, 70 + cur0, NSLOT};
                            RunForm p{}, q{};
                            q.level = level;
                            for (int k = 0; k <= T; ++k) {
                                const StepState s = step_state(e, p, T, k), t = step_state(e, q, T, k);
                                same = same && s.cur == t.cur && s.qcur == t.qcur && s.parity == t.parity && s.n_predict == t.n_predict &&
                                       s.t_index == t.t_index && s.wbuf == t.wbuf && s.w_pingpong == t.w_pingpong;
                                // and is what the stored form's bookkeeping says: planes alternate, one buffer, no ping-pong
                                same = same && t.cur == (cur0 ^ (k & 1)) && t.qcur == (qcur0 ^ 1 ^ (k & 1)) && t.wbuf == 0 && !t.w_pingpong &&
                                       t.parity == (par0 + 1 + k) % NSLOT && t.n_predict == e.n_predict + (uint32_t)k && t.t_index == e.t_index + k;
                            }
                            const StepState s = end_state(e, p, T), t = end_state(e, q, T);
                            same = same && s.cur == t.cur && s.qcur == t.qcur && s.parity == t.parity && s.n_predict == t.n_predict &&
                                   s.t_index == t.t_index && s.wbuf == t.wbuf && s.w_pingpong == t.w_pingpong;
                            same = same && t.qcur == (qcur0 ^ (T & 1)) && t.parity == (par0 + T) % NSLOT;
                        }
        check(same, "steps: the state of every timestep of runs of 1 to 9 steps does not depend on the level");
    }
}

int main() {
    printf("# form\n");       // tests/test_run_plan.py reads the two sections apart
    plan_cases();
    step_cases();
    key_cases();
    printf("# level\n");
    level_cases();
    printf("%d failed\n", failed);
    return failed;
}
