// host/run.hpp — the trajectory loop (forward_trajectory / loglik).  Part of capi.hip (one translation unit).
// The form of a run is decided in host/run_plan.hpp (make_run_plan), in front of the first launch; RunLoop enqueues what the plan says.

// ---- what bank_run and bank_aux_run (host/aux.hpp) share ------------------------------------------------------------------
static bool wants_history(const llpf_run_outputs& o) { return o.x_hist || o.w_hist || o.we_hist; }
static int run_check_args(Bank& b, const double* U, const double* Y, int64_t T, const llpf_run_outputs& o) {
    CHK(use_device(b));
    if (T < 1) return fail(LLPF_ERR_ARG, "T must be >= 1");
    if (!Y) return fail(LLPF_ERR_ARG, "Y is null");
    if (b.nu > 0 && !U) return fail(LLPF_ERR_ARG, "U is null");
    if (wants_history(o) && b.F != 1) return fail(LLPF_ERR_ARG, "history outputs need a single filter");
    return LLPF_OK;
}
// The inputs of a run to the device, laid out [T][FM][nu | ny] with FM = 1, or FM = F for `multi`: every filter of the bank has its own
// inputs, U [F][T][nu] and Y [F][T][ny] (the Monte-Carlo loops of the reference's own benchmark, examples/example_lineargaussian.jl:282-316,
// as one bank); missing measurements must coincide.
static int stage_inputs(Bank& b, const double* U, const double* Y, int64_t T, bool multi) {
    const int FM = multi ? b.F : 1;
    CHK(b.d_U.ensure((size_t)T * FM * (b.nu > 0 ? b.nu : 1)));
    CHK(b.d_Y.ensure((size_t)T * FM * b.ny));
    std::vector<double> stageU, stageY;
    if (multi) {
        if (is_rb(b)) return fail(LLPF_ERR_ARG, "per-filter inputs are not provided for the Rao-Blackwellized model");
        stageY.resize((size_t)T * FM * b.ny);
        for (int f = 0; f < FM; ++f)
            for (int64_t k = 0; k < T; ++k) {
                const double* src = Y + ((size_t)f * T + k) * b.ny;
                if ((src[0] != src[0]) != (Y[(size_t)k * b.ny] != Y[(size_t)k * b.ny])) return fail(LLPF_ERR_ARG, "missing measurements must coincide across the filters of a bank");
                for (int i = 0; i < b.ny; ++i) stageY[((size_t)k * FM + f) * b.ny + i] = src[i];
            }
        if (b.nu > 0) {
            stageU.resize((size_t)T * FM * b.nu);
            for (int f = 0; f < FM; ++f)
                for (int64_t k = 0; k < T; ++k)
                    for (int i = 0; i < b.nu; ++i) stageU[((size_t)k * FM + f) * b.nu + i] = U[((size_t)f * T + k) * b.nu + i];
        }
    }
    if (b.nu > 0) HIPC(hipMemcpyAsync(b.d_U, multi ? stageU.data() : U, sizeof(double) * T * FM * b.nu, hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_Y, multi ? stageY.data() : Y, sizeof(double) * T * FM * b.ny, hipMemcpyHostToDevice, b.stream));
    if (multi) HIPC(hipStreamSynchronize(b.stream));     // the staging vectors are pageable host memory
    return LLPF_OK;
}
// row k of the history, copied out from the normalised state between correct! and predict!:
// x[:,t] .= particles(pf); w[:,t] .= weights(pf); we[:,t] .= expweights(pf)  (reference src/filtering.jl:357-359)
static int copy_history_row(Bank& b, const llpf_run_outputs& o, int64_t k) {
    BankDev d = b.dev();
    auto out = [&](double* hist, size_t row) -> int {      // d_tmp to row k of a history output
        HIPC(hipMemcpyAsync(hist + (size_t)k * row, b.d_tmp, sizeof(double) * row, hipMemcpyDeviceToHost, b.stream));
        HIPC(hipStreamSynchronize(b.stream));
        return LLPF_OK;
    };
    if (o.x_hist) { HIPC(launch_soa2aos(b.devp(), b.d_x[b.cur], b.d_tmp, b.stream)); CHK(out(o.x_hist, (size_t)b.N * b.nxp)); }
    if (o.w_hist) { HIPC(launch_materialize(d, b.d_tmp, nullptr, b.stream)); CHK(out(o.w_hist, (size_t)b.N)); }
    if (o.we_hist) { HIPC(launch_materialize(d, nullptr, b.d_tmp, b.stream)); CHK(out(o.we_hist, (size_t)b.N)); }
    return LLPF_OK;
}
// What a run begins with: zero the running log-likelihood and remember the resample counter.  The device adds `step_base` to every
// Philox step argument (rel_step).
static int run_zero_totals(Bank& b, uint32_t step_base) {
    std::vector<FilterScal> h;
    CHK(scal_download(b, h));
    b.run_resamples = 0;
    b.step_base = step_base;
    for (int f = 0; f < b.F; ++f) { h[f].ll_total = 0.0; h[f].step_base = step_base; b.run_resamples -= h[f].resample_count; }
    return scal_upload(b, h);
}
// what a run ends with, after ev_run1 is recorded and its outputs are on their way: the filters' scalars, the elapsed time, the profile
// and the resample count (the caller subtracted the counters' values at entry)
static int run_finish(Bank& b, std::vector<FilterScal>& h) {
    CHK(scal_download(b, h));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, b.ev_run0, b.ev_run1));
    b.last_run_ms = ms;
    if (b.profiling) prof_collect(b);
    for (int f = 0; f < b.F; ++f) b.run_resamples += h[f].resample_count;
    return LLPF_OK;
}

// ---- the launches of a planned run ----------------------------------------------------------------------------------------
// History outputs are staged on the device (one row per timestep, written between the head and the propagate of the
// balanced form, no host round trip per step) and copied out in bulk at the end; beyond 16 GB of history the
// step-synchronous loop (RunLoop::run_rows) copies row by row instead.
struct HistStage {
    bool on = false;
    size_t rows = 0;
    double *x = nullptr, *w = nullptr, *we = nullptr;
};
static HistStage stage_history(Bank& b, const llpf_run_outputs& o, int64_t T) {
    HistStage hs;
    hs.rows = (size_t)T * b.N;
    const size_t doubles = (o.x_hist ? hs.rows * b.nxp : 0) + (o.w_hist ? hs.rows : 0) + (o.we_hist ? hs.rows : 0);
    // the staging buffer can be most of the device's memory: if it cannot be had, copy row by row instead of failing
    hs.on = wants_history(o) && doubles * sizeof(double) <= ((size_t)16 << 30) && b.d_hist.try_ensure(doubles);
    if (hs.on) {
        double* p = b.d_hist;
        if (o.x_hist) { hs.x = p; p += hs.rows * b.nxp; }
        if (o.w_hist) { hs.w = p; p += hs.rows; }
        if (o.we_hist) { hs.we = p; p += hs.rows; }
    }
    return hs;
}
// LLPF_DEBUG_TIMING: the per-tile clock readings the fused launch of one step left in d_dbg, as text
static int dump_debug_timing(Bank& b, const DevBuf<uint64_t>& d_dbg) {
    std::vector<uint64_t> hd((size_t)8 * b.P2);
    HIPC(hipMemcpyAsync(hd.data(), d_dbg, sizeof(uint64_t) * hd.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    FILE* fp = fopen("gpurun_out/llpf_timing.txt", "w");
    if (fp) {
        for (int t = 0; t < b.P2; ++t) {
            for (int q = 0; q < 8; ++q) fprintf(fp, "%llu ", (unsigned long long)hd[(size_t)t * 8 + q]);
            fprintf(fp, "\n");
        }
        fclose(fp);
    }
    return LLPF_OK;
}

struct RunLoop {
    Bank& b;
    const RunPlan& p;
    const RunSwitches& sw;
    const llpf_run_outputs& o;
    const double* Y;
    const int64_t T;
    const double t_index0;
    const HistStage& hs;
    const RunEntry e;                  // the bank's state at entry
    double* const wbuf[2];             // the weights at entry, and the second buffer of a lazy run (else the same again)
    const int FM, K, ne2;
    const double Ts;

    RunLoop(Bank& bb, const RunPlan& pp, const RunSwitches& s, const llpf_run_outputs& oo, const double* y, int64_t t, double ti0, const HistStage& h)
        : b(bb), p(pp), sw(s), o(oo), Y(y), T(t), t_index0(ti0), hs(h), e{bb.cur, bb.qcur, bb.parity, bb.n_predict, bb.t_index, ACC_NSLOT},
          wbuf{bb.d_w, pp.lazy_run ? bb.d_w_spare : bb.d_w}, FM(pp.multi ? bb.F : 1), K(llpf_qbits(bb.N)), ne2(need_e2(bb)), Ts(bb.cfg.model.Ts) {}

    bool has_y(int64_t k) const { return !(Y[k * b.ny] != Y[k * b.ny]); }
    double tk(int64_t k) const { return (t_index0 + (double)k) * Ts; }
    void enter(const StepState& s) {
        b.cur = s.cur; b.qcur = s.qcur; b.parity = s.parity; b.n_predict = s.n_predict; b.t_index = s.t_index;
        b.d_w = wbuf[s.wbuf];
        if (p.lazy_run) b.d_w_spare = wbuf[s.wbuf ^ 1];
        b.w_pingpong = s.w_pingpong;
    }
    void at_step(int64_t k) { enter(step_state(e, p, T, k)); }

    ResArgs res_args(int64_t k, bool fast) const {
        ResArgs ra{};
        ra.parity = head_slot(e, k); ra.step = rel_step(b); ra.M = (int32_t)b.N; ra.anc_out = b.d_anc;
        ra.accumulate = 1; ra.want_xmean = p.want_xm; ra.u_from_scal = 1; ra.count_surv = p.fx_capable;
        ra.ll_steps = o.ll_steps ? (double*)b.d_ll_steps : nullptr;
        ra.xmean = p.want_xm ? (double*)b.d_xmean : nullptr;
        ra.k = k; ra.row = k; ra.fast_head = fast ? 1 : 0;
        ra.ablate = p.ablate;
        return ra;
    }
    StepArgs step_args(int64_t k) const {
        StepArgs st{};
        st.u = b.nu > 0 ? b.d_U + k * FM * b.nu : nullptr;
        st.u_stride = p.multi ? b.nu : 0; st.y_stride = p.multi ? b.ny : 0;
        st.t_prop = tk(k);
        st.step = rel_step(b);
        st.parity = b.parity;
        st.need_e2 = ne2; st.K = K; st.k = k; st.next_step = rel_step(b) + 1; st.want_xmean = p.want_xm; st.accumulate = p.acc_in_weighting;
        if (is_rb(b)) { st.rb_pred = b.d_rbseq + (size_t)(2 * k + 1) * b.F; st.rb_corr = b.d_rbseq + (size_t)(2 * k + 2) * b.F; }
        const bool weight = (k + 1 < T);
        if (weight) { st.y = b.d_Y + (k + 1) * FM * b.ny; st.t_meas = tk(k + 1); st.has_y = has_y(k + 1) ? 1 : 0; }
        else { st.y = nullptr; st.t_meas = tk(k); st.has_y = 0; }
        return st;
    }
    // the outputs derived from the normalised state of step k, between correct! and predict! (the balanced form leaves it in memory)
    int step_outputs(const BankDev& d, int64_t k) {
        if (p.xm_launch) { ProfScope ps(b, LLPF_PROF_OTHER); CHK(bank_wmean(b, b.d_xmean + (size_t)k * b.nxp)); }
        if (o.xcov) {      // weighted_cov of the state the history would copy out (src/filtering.jl:571-581): mean, then the centred moments
            ProfScope ps(b, LLPF_PROF_OTHER);
            double* mtmp = b.d_xcov + (size_t)T * b.nx * b.nx;
            HIPC(launch_wmean(d, mtmp, b.stream));
            HIPC(launch_wcov(d, mtmp, b.d_xcov + (size_t)k * b.nx * b.nx, b.stream));
        }
        if (o.xquant) {    // the quantiles of the same state: exp-weights materialised, then the radix selection (k_quantile.hip), [t][state][q]
            ProfScope ps(b, LLPF_PROF_OTHER);
            HIPC(launch_materialize(d, nullptr, b.d_wq_we, b.stream));
            HIPC(launch_wquantile(d.xcur, b.Ns, b.nx, b.d_wq_we, b.N, b.d_wq_p, o.nq, b.d_xquant + (size_t)k * b.nx * o.nq, 1, o.nq, b.d_wq, b.stream));
        }
        return LLPF_OK;
    }
    // one timestep in the planned form; `fast`: the head consumes the bound-offset sums of the previous weighting,
    // otherwise the exact-max sums of a k_norm launched just before (redo of a failed step, or a model without a bound)
    int timestep(int64_t k, bool fast, int only_fb) {
        at_step(k);
        BankDev d = b.dev();
        ResArgs ra = res_args(k, fast);
        ra.only_fallback = only_fb;
        StepArgs st = step_args(k);
        st.only_fallback = only_fb;
        const bool weight = (k + 1 < T);
        // (the exact redo of a failed bound test keeps the stored form — and the two weight buffers)
        const bool lazy_q = fast && p.lazy_run && k >= p.k_pp0;
        if (fast && !p.merged) {   // split schedule: the sums of the current weights in bound form, as a streaming launch
            ProfScope ps(b, LLPF_PROF_NORMALISE);
            HIPC(launch_norm(d, ra.parity, p.want_xm, ne2, rel_step(b), 0, lazy_q ? 3 : 1, k, b.stream));
        }
        ra.lazy_q = lazy_q ? 1 : 0;
        ra.level = launch_level(p, fast, weight, k + 2 < T);
        ra.nt_id = p.nt_id;
        if (!fast) {
            ProfScope ps(b, LLPF_PROF_NORMALISE);
            HIPC(launch_norm(d, ra.parity, p.want_xm, 1, rel_step(b), only_fb, 0, k, b.stream));
        }
        if (p.unfused) {
            {
                ra.mode = RES_FINALIZE | RES_RESAMPLE;
                ProfScope ps(b, LLPF_PROF_RESAMPLE);
                if (p.source_fx) { st.marks = 1; HIPC(launch_resample_fx(d, ra, st, b.stream)); }
                else HIPC(launch_resample(d, ra, b.stream));
            }
            CHK(step_outputs(d, k));
            if (hs.on) {
                ProfScope ps(b, LLPF_PROF_OTHER);
                if (hs.x) HIPC(launch_soa2aos(b.devp(), b.d_x[b.cur], hs.x + (size_t)k * b.N * b.nxp, b.stream));
                if (hs.w || hs.we) HIPC(launch_materialize(d, hs.w ? hs.w + (size_t)k * b.N : nullptr, hs.we ? hs.we + (size_t)k * b.N : nullptr, b.stream));
            }
            ProfScope ps(b, LLPF_PROF_PROPAGATE);
            HIPC(launch_step(d, weight ? MODE_PROP_WEIGHT : MODE_PROP, st, b.stream));
        } else {
            DevBuf<uint64_t> d_dbg;
            if (sw.debug_timing && k == sw.debug_step) {
                CHK(d_dbg.ensure((size_t)8 * b.P2));
                HIPC(hipMemsetAsync(d_dbg, 0, sizeof(uint64_t) * 8 * b.P2, b.stream));
                ra.dbg = d_dbg;
            }
            ProfScope ps(b, LLPF_PROF_PROPAGATE);
            HIPC(launch_resprop(d, ra, st, weight ? 1 : 0, b.stream));
            b.last_run_launches += 1;
            if (d_dbg) CHK(dump_debug_timing(b, d_dbg));
        }
        return LLPF_OK;
    }
    // weighting of the first correct! (exp-sums against the bound, quanta, tile sums: no separate normalise pass)
    int first_weighting() {
        enter(entry_state(e));
        BankDev d = b.dev();
        StepArgs a{};
        a.u = b.nu > 0 ? (double*)b.d_U : nullptr; a.y = b.d_Y; a.u_stride = p.multi ? b.nu : 0; a.y_stride = p.multi ? b.ny : 0; a.t_prop = tk(0); a.t_meas = tk(0); a.step = 0; a.has_y = has_y(0) ? 1 : 0;
        a.parity = e.parity; a.need_e2 = ne2; a.K = K; a.k = 0; a.next_step = 0; a.want_xmean = p.want_xm; a.accumulate = p.acc_in_weighting;
        if (is_rb(b)) a.rb_corr = b.d_rbseq;
        ProfScope ps(b, LLPF_PROF_PROPAGATE);
        HIPC(launch_step(d, MODE_WEIGHT, a, b.stream));
        return LLPF_OK;
    }
    // A run whose fused launches store no weights, in front of the exact redo of step kf (>= 1; the weights in front of step 0 are the
    // first weighting's, which stores): the weights of the flagged filters again, by the weighting launch, from the states step kf - 1 left
    // in memory, the measurement of step kf and the prior log(1/N) of a step that resampled — the expression the fused kernel evaluated, on
    // the same doubles.  The launch republishes the slot's bound, uniform and flags with the values they already have.
    int reweight_flagged(int64_t kf) {
        at_step(kf - 1);
        StepArgs st = step_args(kf - 1);                 // the weighting half of the launch that formed them
        st.accumulate = 0; st.want_xmean = 0; st.only_fallback = 1; st.k = kf;
        at_step(kf);
        BankDev d = b.dev();
        ProfScope ps(b, LLPF_PROF_PROPAGATE);
        HIPC(launch_fb_clear(d, 0, 2, b.stream));        // prior of the flagged filters: uniform, log(1/N)
        HIPC(launch_step(d, MODE_WEIGHT, st, b.stream));
        return LLPF_OK;
    }

    // The asynchronous loop as a captured graph, replayed when nothing a launch argument depends on has changed: the key is the
    // plan's form, the run's length, the state at entry, every device buffer a captured launch addresses and which measurements
    // are missing.  `gexec` stays null where the run is to be enqueued.
    int graph_for_run(hipGraphExec_t& gexec) {
        Bank::RunGraph key{};
        key.form = p;
        key.T = T; key.t_index0 = t_index0; key.par0 = e.parity; key.cur0 = e.cur; key.qcur0 = e.qcur;
        key.np_parity = (int)(e.n_predict & 1u);
        key.dU = b.d_U; key.dY = b.d_Y; key.dll = o.ll_steps ? (double*)b.d_ll_steps : nullptr; key.dxm = o.xmean ? (double*)b.d_xmean : nullptr;
        key.dxc = o.xcov ? (double*)b.d_xcov : nullptr; key.drb = b.d_rbseq;
        key.dw = wbuf[0]; key.dws = wbuf[1];
        key.dxq = o.xquant ? (double*)b.d_xquant : nullptr; key.dqp = o.xquant ? (double*)b.d_wq_p : nullptr; key.nq = o.xquant ? o.nq : 0;
        key.yhash = 1469598103934665603ULL;
        for (int64_t k = 0; k < T; ++k) key.yhash = (key.yhash ^ (uint64_t)(has_y(k) ? 1 : 2)) * 1099511628211ULL;
        // a run shape is captured the second time it is seen (capture + instantiation of ~T nodes costs several ms:
        // one-off shapes are simply enqueued)
        Bank::RunGraph* slot = nullptr;
        for (auto& g : b.graphs) if (g.same(key)) { slot = &g; gexec = g.exec.h; break; }
        if (!slot) {
            if (b.graphs.size() >= 4) b.graphs.erase(b.graphs.begin());
            b.graphs.push_back(std::move(key));
        } else if (!gexec) {
            hipGraph_t graph = nullptr;
            auto drop_graph = on_scope_exit([&] { if (graph) hipGraphDestroy(graph); });
            HIPC(hipStreamBeginCapture(b.stream, hipStreamCaptureModeThreadLocal));
            int rc = first_weighting();
            for (int64_t k = 0; rc == LLPF_OK && k < T; ++k) rc = timestep(k, !p.no_bound, 0);
            const hipError_t ee = hipStreamEndCapture(b.stream, &graph);
            CHK(rc);
            if (ee != hipSuccess) return fail(LLPF_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
            const hipError_t ei = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
            if (ei != hipSuccess) return fail(LLPF_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
            slot->exec = GraphExec(gexec);
        }
        return LLPF_OK;
    }

    // Step-synchronous form: the normalised state between correct! and predict! is copied out row by row (history that is not
    // staged on the device).  Same arithmetic as the asynchronous loop (bound-offset form, exact redo when its test fails); not a timed path.
    int run_rows() {
        for (int64_t k = 0; k < T; ++k) {
            at_step(k);
            BankDev d = b.dev();
            ResArgs ra = res_args(k, true);
            ra.mode = RES_FINALIZE;
            HIPC(launch_resample(d, ra, b.stream));
            CHK(redo_if_flagged(b, ra.parity, [&]() -> int {
                b.last_run_redos += 1;
                HIPC(launch_norm(d, ra.parity, p.want_xm, 1, rel_step(b), 1, 0, k, b.stream));
                ra.fast_head = 0; ra.only_fallback = 1;
                HIPC(launch_resample(d, ra, b.stream));
                ra.only_fallback = 0;
                return LLPF_OK;
            }));
            CHK(step_outputs(d, k));
            CHK(copy_history_row(b, o, k));
            ra.mode = RES_RESAMPLE;
            ra.accumulate = 0; ra.ll_steps = nullptr; ra.xmean = nullptr;
            HIPC(launch_resample(d, ra, b.stream));
            StepArgs st = step_args(k);
            HIPC(launch_step(d, (k + 1 < T) ? MODE_PROP_WEIGHT : MODE_PROP, st, b.stream));
        }
        return LLPF_OK;
    }
    // Optimistic enqueue: all remaining timesteps at once, one poll at the end.  Every launch after a failed bound
    // test is a no-op, so when tests fail often (banks of many small filters: some filter fails at most steps) the
    // batch shrinks to a quarter on a failure and doubles again on a clean batch.
    // `replayed`: a graph that holds all T timesteps is on the stream; after a failed bound test the rest is enqueued.
    int run_async(bool replayed) {
        int64_t k0 = 0, batch = T;
        while (k0 < T) {
            const int64_t k1 = replayed ? T : std::min(T, k0 + batch);
            if (!replayed) {
                for (int64_t k = k0; k < k1; ++k) CHK(timestep(k, !p.no_bound, 0));
                test_throw("run_loop");
            }
            replayed = false;
            Flagged fl;
            CHK(poll_fallback(b, fl));
            if (!fl.any) { k0 = k1; batch = std::min(T, batch * 2); continue; }
            // step kf of the flagged filters: exact-max normalisation of the same weights, then the step again
            const int64_t kf = fl.step;
            b.last_run_redos += 1;
            if (p.level >= RUN_SKIP_W && kf > 0) CHK(reweight_flagged(kf));
            CHK(clear_slot_sums(b, head_slot(e, kf)));
            CHK(timestep(kf, false, 1));
            CHK(clear_fallback(b));
            k0 = kf + 1;
            batch = std::max<int64_t>(1, std::min(batch, T) / 4);
        }
        return LLPF_OK;
    }
};

// the whole gain schedule of a run of the Rao-Blackwellized model (data independent): corr_0, pred_0, corr_1, pred_1, ..., [F] each
static int stage_rb_schedule(Bank& b, const double* Y, int64_t T) {
    const size_t need = (size_t)(2 * T + 1) * b.F;
    CHK(b.d_rbseq.ensure(need));
    std::vector<RBStep> seq(need);
    for (int64_t k = 0; k < T; ++k)
        for (int f = 0; f < b.F; ++f) {
            if (!(Y[k * b.ny] != Y[k * b.ny])) CHK(rb_corr_step(b, f, seq[(size_t)(2 * k) * b.F + f]));
            else memset(&seq[(size_t)(2 * k) * b.F + f], 0, sizeof(RBStep));
            CHK(rb_pred_step(b, f, seq[(size_t)(2 * k + 1) * b.F + f]));
        }
    memset(&seq[(size_t)(2 * T) * b.F], 0, sizeof(RBStep) * b.F);
    HIPC(hipMemcpyAsync(b.d_rbseq, seq.data(), sizeof(RBStep) * need, hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// ---- the trajectory loop ------------------------------------------------------------------------
// ll_total [F]; of `o`: ll_steps [T][F], xmean [T][F][nx], xcov [T][nx][nx], xquant [T][nx][nq], quant_p [nq]; `multi`: stage_inputs
static int bank_run(Bank& b, const double* U, const double* Y, int64_t T, double t_index0, double* ll_total, const llpf_run_outputs& o, bool multi = false) {
    // 1. the arguments
    CHK(run_check_args(b, U, Y, T, o));
    test_throw("run");
    const bool rbfull = is_rbfull(b);
    if (o.xcov && (b.F != 1 || rbfull)) return fail(LLPF_ERR_ARG, "the xcov output needs a single filter that is not LLPF_MODEL_RB_BILINEAR");
    if (o.xquant) {
        if (b.F != 1 || rbfull) return fail(LLPF_ERR_ARG, "the xquant output needs a single filter that is not LLPF_MODEL_RB_BILINEAR");
        if (!o.quant_p || o.nq < 1 || o.nq > 1024) return fail(LLPF_ERR_ARG, "the xquant output needs 1 <= nq <= 1024 probabilities");
        for (int i = 0; i < o.nq; ++i) if (!(o.quant_p[i] >= 0.0 && o.quant_p[i] <= 1.0)) return fail(LLPF_ERR_ARG, "xquant: a probability outside [0, 1]");
    }
    if (o.xmean && rbfull && b.F != 1) return fail(LLPF_ERR_ARG, "weighted means of a BANK of filters with per-particle covariance are not provided (run without xmean)");

    // 2. the inputs, and the filters' scalars
    b.aux_pending = false; b.we_is_lambda = false;
    CHK(stage_inputs(b, U, Y, T, multi));
    if (is_rb(b)) CHK(stage_rb_schedule(b, Y, T));
    CHK(run_zero_totals(b, b.n_predict));      // the launches of a run carry relative steps 0, 1, ...

    // 3. the plan
    RunFacts facts;
    facts.model_id = b.cfg.model.model_id; facts.nx = b.nx; facts.F = b.F; facts.P2 = b.P2; facts.Ns = b.Ns;
    facts.strategy = b.cfg.resampling_strategy; facts.thr = b.cfg.resample_threshold;
    facts.traits = facts.model_id >= LLPF_MODEL_USER_BASE ? jit_model_traits(facts.model_id) : 0;
    facts.fx_supported = resample_fx_supported(facts.model_id, b.nx, b.ny, facts.strategy);
    facts.hist = wants_history(o); facts.xmean = o.xmean; facts.xcov = o.xcov; facts.xquant = o.xquant; facts.ll_steps = o.ll_steps; facts.multi = multi;
    facts.profiling = b.profiling; facts.T = T; facts.surv_frac = b.surv_frac; facts.use_fx = b.use_fx;
    facts.sw = read_run_switches();
    const RunPlan plan = make_run_plan(facts);
    b.use_fx = plan.use_fx;
    b.last_run_launches = 0; b.last_run_fx_steps = plan.source_fx ? T : 0; b.last_run_surv = -1.0;
    b.last_run_level = plan.level; b.last_run_skip_max = plan.skip_max; b.last_run_redos = 0;

    // 4. what the plan needs
    if (o.ll_steps) CHK(b.d_ll_steps.ensure((size_t)T * b.F));
    if (o.xmean) CHK(b.d_xmean.ensure((size_t)T * b.F * b.nxp));
    if (plan.want_xm) CHK(ensure_xmpart(b));
    if (o.xcov) CHK(b.d_xcov.ensure((size_t)T * b.nx * b.nx + MAXD));
    if (o.xquant) {      // weighted_quantile(sol, q) (src/filtering.jl:583-595) of the state the history would copy out, per timestep, on the device
        CHK(ensure_wq(b, o.quant_p, o.nq));
        HIPC(hipStreamSynchronize(b.stream));
        CHK(b.d_xquant.ensure((size_t)T * b.nx * o.nq));
    }
    const size_t n_surv = (size_t)b.F * b.P2 * 4;
    if (plan.fx_capable) {
        CHK(b.d_surv.ensure(n_surv));
        HIPC(hipMemsetAsync(b.d_surv, 0, sizeof(unsigned long long) * n_surv, b.stream));
    }
    if (plan.source_fx) CHK(ensure_fx(b));
    if (plan.lazy_run && !b.d_w_spare) {      // the second weight buffer starts as a copy, so that its padding holds -Inf too
        if (!b.d_w_alloc.try_ensure((size_t)b.F * b.Ns)) return fail(LLPF_ERR_ALLOC, "second weight buffer of the split schedule");
        b.d_w_spare = b.d_w_alloc;
        HIPC(hipMemcpyAsync(b.d_w_spare, b.d_w, sizeof(double) * (size_t)b.F * b.Ns, hipMemcpyDeviceToDevice, b.stream));
    }
    const HistStage hs = stage_history(b, o, T);
    RunLoop run(b, plan, facts.sw, o, Y, T, t_index0, hs);
    // however the run ends (a failed status or a throw included), the verbs after it weight in place, on the buffer it began in
    auto restore_w = on_scope_exit([&] {
        b.d_w = run.wbuf[0];
        if (plan.lazy_run) b.d_w_spare = run.wbuf[1];
        b.w_pingpong = false;
    });

    // 5. capture, replay or enqueue
    hipGraphExec_t gexec = nullptr;
    if (plan.use_graph) CHK(run.graph_for_run(gexec));
    HIPC(hipEventRecord(b.ev_run0, b.stream));
    if (gexec) { HIPC(hipGraphLaunch(gexec, b.stream)); b.last_run_launches = T; }
    else CHK(run.first_weighting());
    if (facts.hist && !hs.on) CHK(run.run_rows());
    else CHK(run.run_async(gexec != nullptr));

    // 6. the state the run leaves, and its outputs
    run.enter(end_state(run.e, plan, T));
    {
        BankDev d = b.dev();
        ProfScope ps(b, LLPF_PROF_OTHER);
        // the run's k_norm launches stored no quanta: leave those of the current weights behind, as every later verb expects them
        if (plan.lazy_run) HIPC(launch_requant(d, b.stream));
        HIPC(launch_post_predict(d, b.stream));
    }
    HIPC(hipEventRecord(b.ev_run1, b.stream));
    if (hs.on) {
        if (o.x_hist) HIPC(hipMemcpyAsync(o.x_hist, hs.x, sizeof(double) * hs.rows * b.nxp, hipMemcpyDeviceToHost, b.stream));
        if (o.w_hist) HIPC(hipMemcpyAsync(o.w_hist, hs.w, sizeof(double) * hs.rows, hipMemcpyDeviceToHost, b.stream));
        if (o.we_hist) HIPC(hipMemcpyAsync(o.we_hist, hs.we, sizeof(double) * hs.rows, hipMemcpyDeviceToHost, b.stream));
    }
    if (hs.on && b.d_hist.cap * sizeof(double) > ((size_t)256 << 20)) {
        // a large history staging buffer is not kept for the lifetime of the handle (other filters / banks need the memory)
        HIPC(hipStreamSynchronize(b.stream));
        b.d_hist.reset();
    }
    if (o.ll_steps) HIPC(hipMemcpyAsync(o.ll_steps, b.d_ll_steps, sizeof(double) * T * b.F, hipMemcpyDeviceToHost, b.stream));
    if (o.xmean) HIPC(hipMemcpyAsync(o.xmean, b.d_xmean, sizeof(double) * T * b.F * b.nxp, hipMemcpyDeviceToHost, b.stream));
    if (o.xcov) HIPC(hipMemcpyAsync(o.xcov, b.d_xcov, sizeof(double) * T * b.nx * b.nx, hipMemcpyDeviceToHost, b.stream));
    if (o.xquant) HIPC(hipMemcpyAsync(o.xquant, b.d_xquant, sizeof(double) * T * b.nx * o.nq, hipMemcpyDeviceToHost, b.stream));
    std::vector<FilterScal> h;
    CHK(run_finish(b, h));
    if (ll_total) for (int f = 0; f < b.F; ++f) ll_total[f] = h[f].ll_total;
    if (plan.fx_capable) {      // the sources whose f the run's steps needed: what the next run's form is chosen by (make_run_plan)
        double surv = 0.0;
        std::vector<unsigned long long> hsv(n_surv);
        HIPC(hipMemcpy(hsv.data(), b.d_surv, sizeof(unsigned long long) * n_surv, hipMemcpyDeviceToHost));
        for (unsigned long long v : hsv) surv += (double)v;
        b.last_run_surv = b.surv_frac = surv / ((double)T * (double)b.N * (double)b.F);
    }
    return check_status(b, h);
}
