// host/fallback.hpp — host side of a failed bound test (exact-max redo).  Part of capi.hip (one translation unit).
// ---- exact-form redo of a normalisation whose bound test failed ------------------------------------------------
// zero the exp-sum words of accumulator slot `slot` for the filters whose fallback flag is set (on the device: a bank of
// thousands of small filters may flag most of them at once)
static int clear_slot_sums(Bank& b, int slot) {
    HIPC(launch_fb_clear(b.dev(), slot, 0, b.stream));
    return LLPF_OK;
}
// did some filter ask for the exact form, and at which run-step?  Clears nothing.  Which filters is known to the device
// (FilterScal::fallback); the host only needs "some".
struct Flagged { bool any = false; int64_t step = -1; };
static int poll_fallback(Bank& b, Flagged& fl) {
    uint32_t flag = 0;
    HIPC(hipMemcpyAsync(&flag, b.d_flag, sizeof(flag), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    fl.any = flag != 0;
    fl.step = (int64_t)flag - 1;
    return LLPF_OK;
}
static int clear_fallback(Bank& b) {
    HIPC(launch_fb_clear(b.dev(), 0, 1, b.stream));
    return LLPF_OK;
}
// The redo of one launch sequence whose sums went to `slot`: if some filter's bound test failed, `exact` enqueues the exact-max
// normalisation of the same weights and the sequence again for the flagged filters (only_fallback = 1).
template <class Exact>
static int redo_if_flagged(Bank& b, int slot, Exact exact) {
    Flagged fl;
    CHK(poll_fallback(b, fl));
    if (!fl.any) return LLPF_OK;
    CHK(clear_slot_sums(b, slot));
    CHK(exact());
    return clear_fallback(b);
}
static int need_e2(const Bank& b) { return b.cfg.resample_threshold != 1.0 ? 1 : 0; }
