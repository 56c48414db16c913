// run_plan_skip_anc_host.cpp — RunForm::skip_anc_run (csrc/host/run_plan.hpp) checked without a device (tests/test_run_plan_skip_anc.py):
// a run whose fused launches store no weights stores no ancestors between its steps either, LLPF_SKIP_ANC=0 pins the storing form, the
// field is part of the key of a captured graph, and the step bookkeeping does not depend on it.  The expected values are the rule written
// out by hand: skip_w_run's preconditions (fused, merged schedule with sums in the weighting, not Rao-Blackwellized, threshold exactly 1,
// more than one tile) and the switch.
// Build: c++ -std=c++17 run_plan_skip_anc_host.cpp -o run_plan_skip_anc_host
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

static const int64_t TILE = 1024;
static const int NSLOT = 3;            // ACC_NSLOT (csrc/engine.hpp)

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
        const RunPlan p = make_run_plan(lg(M, 1.0));
        CHECK(p.skip_w_run && p.skip_anc_run);
        CHECK(p.skip_w_run == 1 && p.skip_anc_run == 1);
    }
    CHECK(!make_run_plan(lg(M, 0.1)).skip_anc_run);
    CHECK(!make_run_plan(lg(M, 0.999999)).skip_anc_run);
    CHECK(make_run_plan(lg((int64_t)3 << 20, 1.0)).skip_anc_run);
    CHECK(!make_run_plan(lg(((int64_t)3 << 20) + TILE, 1.0)).skip_anc_run);      // the split schedule
    {
        RunFacts f = lg(M, 1.0); f.P2 = 1;
        CHECK(!make_run_plan(f).skip_anc_run);                                   // one tile
        f.P2 = 2;
        CHECK(make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_RB_LINEAR;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_QUADTANK_RK4; f.nx = 4;
        CHECK(!make_run_plan(f).skip_anc_run);                                   // the balanced form
        f = lg(M, 1.0); f.nx = 3;
        CHECK(!make_run_plan(f).skip_anc_run);
        f.sw.unfused = 0;
        CHECK(make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.strategy = LLPF_RESAMPLE_RESIDUAL;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.strategy = LLPF_RESAMPLE_STRATIFIED;
        CHECK(make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.hist = true;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.xcov = true;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.xquant = true;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.xmean = true; f.ll_steps = true; f.multi = true;
        CHECK(make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.sw.schedule = 0;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(M, 1.0); f.model_id = LLPF_MODEL_USER_BASE + 3; f.traits = LLPF_TRAIT_LOGLIK;
        CHECK(!make_run_plan(f).skip_anc_run);
        f = lg(TILE, 1.0); f.F = 3 << 10;                                        // a bank in the merged schedule
        CHECK(make_run_plan(f).skip_anc_run == make_run_plan(f).skip_w_run);
    }
    name = "switches";
    {
        RunFacts f = lg(M, 1.0);
        f.sw.skip_anc = 0;
        CHECK(make_run_plan(f).skip_w_run && !make_run_plan(f).skip_anc_run);    // the storing form of the same run
        f.sw.skip_anc = 1;
        CHECK(make_run_plan(f).skip_w_run && make_run_plan(f).skip_anc_run);
        f.sw.skip_w = 0;
        CHECK(!make_run_plan(f).skip_w_run && !make_run_plan(f).skip_anc_run);   // never without skip_w_run
        f = lg(M, 0.1); f.sw.skip_anc = 1;
        CHECK(!make_run_plan(f).skip_anc_run);                                   // the switch pins the storing form; it cannot force the other
        // every shape: the field is skip_w_run's answer and the switch
        bool follows = true;
        for (int thr1 = 0; thr1 < 2; ++thr1)
            for (int P2 = 1; P2 <= 2; ++P2)
                for (int rb = 0; rb < 2; ++rb)
                    for (int unf = -1; unf <= 1; ++unf)
                        for (int sch = -1; sch <= 1; ++sch)
                            for (int sw = -1; sw <= 1; ++sw)
                                for (int sa = -1; sa <= 1; ++sa) {
                                    RunFacts g = lg(M, thr1 ? 1.0 : 0.5);
                                    g.P2 = P2; g.model_id = rb ? LLPF_MODEL_RB_LINEAR : LLPF_MODEL_LINEAR_GAUSSIAN;
                                    g.sw.unfused = unf; g.sw.schedule = sch; g.sw.skip_w = sw; g.sw.skip_anc = sa;
                                    const RunPlan p = make_run_plan(g);
                                    const bool fused = unf != 1, merged = sch != 0;
                                    const bool w = fused && merged && !rb && thr1 && P2 > 1 && sw != 0;
                                    follows = follows && (p.skip_w_run != 0) == w && (p.skip_anc_run != 0) == (w && sa != 0);
                                }
        check(follows, "switches: skip_anc_run == skip_w_run's preconditions && LLPF_SKIP_ANC != 0, over 648 shapes");
    }
    name = "environment";
    {
        CHECK(read_run_switches().skip_anc == -1);
        setenv("LLPF_SKIP_ANC", "0", 1);
        CHECK(read_run_switches().skip_anc == 0);
        RunFacts f = lg(M, 1.0);
        f.sw = read_run_switches();
        CHECK(make_run_plan(f).skip_w_run && !make_run_plan(f).skip_anc_run);
        setenv("LLPF_SKIP_ANC", "1", 1);
        CHECK(read_run_switches().skip_anc == 1);
        unsetenv("LLPF_SKIP_ANC");
        CHECK(read_run_switches().skip_anc == -1);
    }
}

static void key_cases() {
    const char* name = "graph key";
    RunFacts f = lg((int64_t)1 << 20, 1.0);
    const RunForm a = make_run_plan(f);
    f.sw.skip_anc = 0;
    const RunForm b = make_run_plan(f);
    CHECK(!(a == b));
    RunForm c = b;
    c.skip_anc_run = 1;                               // they differ in nothing else
    CHECK(c == a);
    c = a; c.skip_anc_run = 0;
    CHECK(c == b && !(c == a));
    c = a; c.skip_w_run = 0;
    CHECK(!(c == a) && c.skip_anc_run == 1);          // neither field spills into the other
}

// the host-side state of every timestep is the same with and without the field
static void step_cases() {
    bool same = true;
    for (int T = 1; T <= 9; ++T)
        for (int par0 = 0; par0 < NSLOT; ++par0)
            for (int cur0 = 0; cur0 < 2; ++cur0)
                for (int qcur0 = 0; qcur0 < 2; ++qcur0) {
                    const RunEntry e{cur0, qcur0, par0, 1000u + (uint32_t)par0, 70 + cur0, NSLOT};
                    RunForm p{}, q{};
                    p.skip_w_run = 1; q.skip_w_run = 1; q.skip_anc_run = 1;
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
    check(same, "steps: the state of every timestep of runs of 1 to 9 steps does not depend on skip_anc_run");
}

int main() {
    plan_cases();
    key_cases();
    step_cases();
    printf("%d failed\n", failed);
    return failed;
}
