// tail_acc_host.cpp — which launches of a run at resample_threshold 1 leave no running maximum (csrc/host/run_plan.hpp: RunKey::skip_max,
// RUN_NO_MAX, launch_level with a plan), checked without a device (tests/test_tail_acc_plan.py).  A host compiler alone builds this
// program.  The expected values are the rule written out by hand, never the output of the code under test.
// Build: c++ -std=c++17 -fsanitize=address,undefined tail_acc_host.cpp -o tail_acc_host
// Prints one line per check; the exit status is the number of failed checks.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../lowlevelparticlefilters.jl_amd/csrc/host/run_plan.hpp"

static int failed = 0;
static void check(bool ok, const std::string& what) {
    printf("%s %s\n", ok ? "ok  " : "FAIL", what.c_str());
    if (!ok) ++failed;
}
#define CHECK(cond) check((cond), std::string(name) + ": " #cond)

// the headline workload: linear-Gaussian, nx = 2, one filter of 2^20 particles, no output asked for
static RunFacts lg(double thr) {
    RunFacts f;
    f.model_id = LLPF_MODEL_LINEAR_GAUSSIAN; f.nx = 2; f.F = 1; f.Ns = (int64_t)1 << 20; f.P2 = 1024;
    f.strategy = LLPF_RESAMPLE_SYSTEMATIC; f.thr = thr; f.T = 10;
    return f;
}

int main() {
    const char* name = "levels";
    CHECK(RUN_LEAN == 3 && RUN_NO_MAX == 4 && LLPF_SKIP_MAX == 1);

    // the plan: skip_max exactly where the level is 3 and LLPF_SKIP_MAX is not 0; the plan's level itself never exceeds 3
    name = "plan";
    {
        CHECK(make_run_plan(lg(1.0)).level == 3 && make_run_plan(lg(1.0)).skip_max == 1);
        CHECK(make_run_plan(lg(0.5)).level == 0 && make_run_plan(lg(0.5)).skip_max == 0);
        bool follows = true, capped = true;
        int shapes = 0;
        const int strategies[3] = {LLPF_RESAMPLE_SYSTEMATIC, LLPF_RESAMPLE_STRATIFIED, LLPF_RESAMPLE_RESIDUAL};
        const int models[3] = {LLPF_MODEL_LINEAR_GAUSSIAN, LLPF_MODEL_RB_LINEAR, LLPF_MODEL_QUADTANK_RK4};
        for (int si = 0; si < 3; ++si)
            for (int xm = 0; xm < 2; ++xm)
                for (int thr1 = 0; thr1 < 2; ++thr1)
                    for (int P2 = 1; P2 <= 2; ++P2)
                        for (int mi = 0; mi < 3; ++mi)
                            for (int nx = 1; nx <= 3; ++nx)
                                for (int sw = -1; sw <= 1; ++sw)
                                    for (int sa = -1; sa <= 1; ++sa)
                                        for (int ln = -1; ln <= 1; ++ln)
                                            for (int sm = -1; sm <= 1; ++sm, ++shapes) {
                                                RunFacts g = lg(thr1 ? 1.0 : 0.5);
                                                g.strategy = strategies[si]; g.xmean = xm != 0; g.P2 = P2; g.model_id = models[mi];
                                                g.nx = models[mi] == LLPF_MODEL_QUADTANK_RK4 ? 4 : nx;
                                                g.sw.skip_w = sw; g.sw.skip_anc = sa; g.sw.lean = ln; g.sw.skip_max = sm;
                                                const RunPlan p = make_run_plan(g);
                                                // level 3 by hand: fused (systematic or stratified, LinGauss below three states), threshold 1, several
                                                // tiles, none of the three switches 0, systematic, no means
                                                const bool lean = models[mi] == LLPF_MODEL_LINEAR_GAUSSIAN && nx <= 2 && strategies[si] == LLPF_RESAMPLE_SYSTEMATIC &&
                                                                  !xm && thr1 && P2 > 1 && sw != 0 && sa != 0 && ln != 0;
                                                follows = follows && (p.level == 3) == lean && p.skip_max == ((lean && sm != 0) ? 1 : 0);
                                                capped = capped && p.level <= RUN_LEAN;
                                            }
        check(follows && shapes == 3 * 2 * 2 * 2 * 3 * 3 * 81, "plan: skip_max == (level 3 && LLPF_SKIP_MAX != 0), over 17496 shapes");
        check(capped, "plan: no plan's level is above RUN_LEAN");
        RunFacts f = lg(1.0);
        f.ll_steps = true; f.multi = true;
        CHECK(make_run_plan(f).skip_max == 1);            // outputs that are not means do not matter
        f = lg(1.0); f.P2 = 2;
        CHECK(make_run_plan(f).skip_max == 1);            // nor the number of tiles, from two on
    }
    name = "environment";
    {
        CHECK(read_run_switches().skip_max == -1);
        setenv("LLPF_SKIP_MAX", "0", 1);
        CHECK(read_run_switches().skip_max == 0);
        RunFacts f = lg(1.0);
        f.sw = read_run_switches();
        CHECK(make_run_plan(f).level == 3 && make_run_plan(f).skip_max == 0);
        setenv("LLPF_SKIP_MAX", "1", 1);
        CHECK(read_run_switches().skip_max == 1);
        unsetenv("LLPF_SKIP_MAX");
        CHECK(read_run_switches().skip_max == -1);
    }
    // one launch: 4 only for a level-3 launch (fast, with a weighting phase) of a plan with skip_max that another weighting launch follows;
    // every other combination is what launch_level without the plan's extras gives
    name = "launch_level";
    {
        const int base[4][2][2] = {      // [level][fast][weight], as tests/run_plan_host.cpp has it
            {{0, 0}, {0, 0}},
            {{0, 0}, {1, 1}},
            {{0, 0}, {1, 2}},
            {{0, 0}, {1, 3}},
        };
        bool ok = true;
        int n = 0;
        for (int level = 0; level < 4; ++level)
            for (int sm = 0; sm < 2; ++sm)
                for (int fast = 0; fast < 2; ++fast)
                    for (int weight = 0; weight < 2; ++weight)
                        for (int next = 0; next < 2; ++next, ++n) {
                            RunKey p{};
                            p.level = level; p.skip_max = sm;
                            const int want = (level == 3 && sm && fast && weight && next) ? 4 : base[level][fast][weight];
                            ok = ok && launch_level(p, fast != 0, weight != 0, next != 0) == want;
                            ok = ok && launch_level(static_cast<const RunForm&>(p), fast != 0, weight != 0) == base[level][fast][weight];
                        }
        check(ok && n == 64, "launch_level: every (level, skip_max, fast, weight, next_weight)");
    }
    // the launches of whole runs, as RunLoop::timestep asks for them: weight = k + 1 < T, next_weight = k + 2 < T
    name = "runs";
    {
        const std::vector<std::vector<int>> want = {{1}, {3, 1}, {4, 3, 1}, {4, 4, 3, 1}, {4, 4, 4, 3, 1}, {4, 4, 4, 4, 3, 1}};
        bool ok = true, off = true, redo = true;
        for (int T = 1; T <= 6; ++T) {
            RunFacts f = lg(1.0);
            f.T = T;
            const RunPlan p = make_run_plan(f);
            f.sw.skip_max = 0;
            const RunPlan q = make_run_plan(f);
            for (int k = 0; k < T; ++k) {
                ok = ok && launch_level(p, true, k + 1 < T, k + 2 < T) == want[T - 1][k];
                off = off && launch_level(q, true, k + 1 < T, k + 2 < T) == (k + 1 < T ? 3 : 1);
                redo = redo && launch_level(p, false, k + 1 < T, k + 2 < T) == 0;      // the exact redo of a failed bound test stores and leaves its maximum
            }
        }
        check(ok, "runs: T = 1 .. 6 are [1], [3 1], [4 3 1], ... — the last weighting launch keeps its maximum, the last launch is level 1");
        check(off, "runs: LLPF_SKIP_MAX=0 leaves every weighting launch at level 3");
        check(redo, "runs: the exact redo is level 0 wherever it falls");
    }
    // the key of a captured graph (Bank::RunGraph holds a RunKey): skip_max tells two keys apart, and so does every field below it
    name = "key";
    {
        RunFacts f = lg(1.0);
        const RunKey a = make_run_plan(f);
        f.sw.skip_max = 0;
        const RunKey b = make_run_plan(f);
        CHECK(a == a && b == b && !(a == b));
        RunKey c = b;
        c.skip_max = a.skip_max;
        CHECK(c == a && !(c == b));
        c = a; c.level = 2;
        CHECK(!(c == a));
        c = a; c.ablate = 128;
        CHECK(!(c == a));
        CHECK(sizeof(RunKey) == sizeof(RunForm) + sizeof(int));
    }
    printf("%d failed\n", failed);
    return failed;
}
