// run_plan_lean_host.cpp — RunForm::lean_run (csrc/host/run_plan.hpp) checked without a device (tests/test_run_plan_lean.py): a run at
// resample_threshold 1 whose fused launches store neither weights nor ancestors, which resamples systematically and wants no weighted
// means, takes the kernel with those facts compiled in (k_resprop<..., LEAN>); LLPF_LEAN=0 pins the kernel with the run-time tests; the
// field is part of the key of a captured graph and shares skip_w_run's int.  The expected values are the rule written out by hand.
// Build: c++ -std=c++17 -fsanitize=address,undefined run_plan_lean_host.cpp -o run_plan_lean_host
// Prints one line per check; the exit status is the number of failed checks.
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

static RunFacts lg(int64_t FNs, double thr) {
    RunFacts f;
    f.model_id = LLPF_MODEL_LINEAR_GAUSSIAN; f.nx = 2; f.F = 1; f.Ns = FNs; f.P2 = 8;
    f.strategy = LLPF_RESAMPLE_SYSTEMATIC; f.thr = thr; f.T = 10;
    return f;
}

static void plan_cases() {
    const int64_t M = (int64_t)1 << 20;
    const char* name = "preconditions";
    {
        const RunPlan p = make_run_plan(lg(M, 1.0));      // the headline workload
        CHECK(p.skip_w_run == 1 && p.skip_anc_run == 1 && p.lean_run == 1 && p.lean_form());
    }
    CHECK(!make_run_plan(lg(M, 0.5)).lean_run && !make_run_plan(lg(M, 0.5)).lean_form());
    CHECK(!make_run_plan(lg(M, 0.999999)).lean_form());
    {
        RunFacts f = lg(M, 1.0); f.strategy = LLPF_RESAMPLE_STRATIFIED;
        CHECK(make_run_plan(f).skip_anc_run && !make_run_plan(f).lean_run && !make_run_plan(f).lean_form());
        f = lg(M, 1.0); f.xmean = true;
        CHECK(make_run_plan(f).skip_anc_run && make_run_plan(f).want_xm && !make_run_plan(f).lean_form());
        f = lg(M, 1.0); f.P2 = 1;
        CHECK(!make_run_plan(f).lean_form());                                    // one tile
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_RB_LINEAR;
        CHECK(!make_run_plan(f).lean_form());
        f = lg(M, 1.0); f.ll_steps = true; f.multi = true;
        CHECK(make_run_plan(f).lean_form());                                     // outputs that are not means do not matter
    }
    name = "switches";
    {
        RunFacts f = lg(M, 1.0);
        f.sw.lean = 0;
        CHECK(make_run_plan(f).skip_anc_run && !make_run_plan(f).lean_run && !make_run_plan(f).lean_form());      // the same run, the kernel with the tests
        f.sw.lean = 1;
        CHECK(make_run_plan(f).lean_form());
        f.sw.skip_anc = 0;
        CHECK(!make_run_plan(f).lean_form());                                    // never where the ancestors are stored
        f = lg(M, 1.0); f.sw.skip_w = 0;
        CHECK(!make_run_plan(f).lean_run && !make_run_plan(f).lean_form());      // ... or the weights
        f = lg(M, 0.5); f.sw.lean = 1;
        CHECK(!make_run_plan(f).lean_form());                                    // the switch pins the other kernel; it cannot force this one
        // every shape: the launches are lean where the run stores no ancestors, resamples systematically, wants no means and LLPF_LEAN != 0
        bool follows = true;
        int shapes = 0;
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
                                    const bool lean = w && sa != 0 && strategies[si] == LLPF_RESAMPLE_SYSTEMATIC && !xm && ln != 0;
                                    follows = follows && (p.skip_w_run != 0) == w && (p.skip_anc_run != 0) == (w && sa != 0) && p.lean_form() == lean;
                                    follows = follows && (!p.lean_run || p.skip_w_run) && (p.lean_run == 0 || p.lean_run == 1);
                                }
        check(follows && shapes == 648, "switches: lean_form() == skip_anc_run && systematic && !xmean && LLPF_LEAN != 0, over 648 shapes");
    }
    name = "environment";
    {
        unsetenv("LLPF_LEAN");
        CHECK(read_run_switches().lean == -1);
        setenv("LLPF_LEAN", "0", 1);
        CHECK(read_run_switches().lean == 0);
        RunFacts f = lg(M, 1.0);
        f.sw = read_run_switches();
        CHECK(make_run_plan(f).skip_anc_run && !make_run_plan(f).lean_form());
        setenv("LLPF_LEAN", "1", 1);
        CHECK(read_run_switches().lean == 1);
        unsetenv("LLPF_LEAN");
        CHECK(read_run_switches().lean == -1);
    }
}

static void key_cases() {
    const char* name = "graph key";
    CHECK(sizeof(RunForm) == 17 * sizeof(int));       // the field took no int of its own
    RunFacts f = lg((int64_t)1 << 20, 1.0);
    const RunForm a = make_run_plan(f);
    f.sw.lean = 0;
    const RunForm b = make_run_plan(f);
    CHECK(!(a == b));
    RunForm c = b;
    c.lean_run = 1;                                   // they differ in nothing else
    CHECK(c == a);
    c = a; c.lean_run = 0;
    CHECK(c == b && !(c == a));
    c = a; c.skip_w_run = 0;
    CHECK(!(c == a) && c.skip_anc_run == 1 && c.lean_run == 1);      // no field spills into another
    c = a; c.skip_anc_run = 0;
    CHECK(!(c == a) && c.skip_w_run == 1 && c.lean_run == 1 && !c.lean_form());
    c = a; c.lean_run = 0;
    CHECK(c.skip_w_run == 1 && c.skip_anc_run == 1);
    // a plan that differs only in LLPF_SKIP_ANC still differs only in skip_anc_run
    f = lg((int64_t)1 << 20, 1.0); f.sw.skip_anc = 0;
    c = make_run_plan(f);
    CHECK(!(c == a));
    c.skip_anc_run = 1;
    CHECK(c == a);
}

int main() {
    plan_cases();
    key_cases();
    printf("%d failed\n", failed);
    return failed;
}
