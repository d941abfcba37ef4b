// lap_wide_drv.hip -- the wide solver's HOST DRIVER (lap_wide.hip describes the solver and holds its searches; lap_wide_rr.hip its
// row reduction): wide_solve_batch sets up the problems' argument blocks and buffers (the layout: lap_wide_dev.h) and enqueues the
// phases; wide_info and wide_note_status report a finished solve; the process-wide counters.
#include "lap_wide_dev.h"

namespace cyto {

static std::atomic<long long> g_embedded_solves{0};    // solves of this process whose searches ran in the embedded form
static std::atomic<long long> g_aborted_searches{0};   // searches of this process that several-searches-at-once solves ended early

static std::atomic<int> g_par_busy[64];     // per device: a several-searches-at-once kernel (wide_aug<..,PAR>) is in flight

int wide_solve_batch(const WidePlan &pl, const std::vector<SolveJob> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                     hipEvent_t ev_arr_done) {
    const int n = pl.n, nl = (int)jobs.size();
    if (!nl) return CYTO_OK;
    int rc;
    auto build_caches_of = [&](const int32_t *flags) -> int {    // flags: per problem, 0 = nothing left to do for it (or null: all)
        for (int k = 0; k < nl; k++) {
            if (flags && flags[k] == 0) continue;
            const SolveJob &j = jobs[(size_t)k];
            const int r = build_caches(pl.cache, n, j.ld, j.cost, j.rowmap, j.fws, j.cache_col, j.cache_val, j.same, stream);
            if (r) return r;
        }
        return CYTO_OK;
    };
    if (nl == 1 && jobs[0].first_count >= 0) {                 // the first caches exist but for the listed rows (lap_jv.hip: fused_fixup)
        const SolveJob &j = jobs[0];
        if ((rc = build_caches(pl.cache, n, j.ld, j.cost, j.rowmap, j.fws, j.cache_col, j.cache_val, j.same, stream, j.first_rows, j.first_count)))
            return rc;
    } else if ((rc = build_caches_of(nullptr))) return rc;
    CYTO_HIP(hipEventRecord(ev_cache_done, stream));
    struct ParSlot { std::atomic<int> *p = nullptr; ~ParSlot() { if (p) p->store(0); } } par_slot;       // (released on every return path)
    int dev_now = 0;
    (void)hipGetDevice(&dev_now);
    const int device_slot = dev_now >= 0 && dev_now < 64 ? dev_now : 0;
    const size_t nT = (size_t)n * sizeof(float);
    const int embed_knob = CYTO_KNOB("CYTO_AUG_EMBED").set ? CYTO_KNOB("CYTO_AUG_EMBED").value : 1;
    std::vector<WideArgs> h_wa((size_t)nl);
    for (int k = 0; k < nl; k++) {
        const SolveJob &j = jobs[(size_t)k];
        // Several searches of ONE problem at once (wide_aug<.., PAR>): by default for a single problem without runs of identical rows
        // from 2 048 rows on (runs of identical rows -- a Visium problem's slots: a tenth as many groups as rows -- finish most of their
        // searches as runs of one-edge steps in the one-workgroup kernel; a sub-spot chunk's few doubled spots do not matter).
        // Its workgroups meet at hand-rolled grid barriers and it is launched as a plain kernel: they must all be RESIDENT, one
        // 1024-thread workgroup per CU.  So G is clamped to the CUs of one XCD, and ONE such kernel runs per device at a time: workgroups
        // of two of them could each get partly scheduled and spin for the rest.  A solve that finds the slot taken runs one search at a
        // time on one workgroup (same results).
        const int xcd_cus = std::max(1, pl.cache.cus / 8);
        const bool dup_rows = n >= 2 && (long long)j.ngroups * 5 < (long long)n * 4;
        int parg = nl != 1 ? 0 : (pl.par > 0 ? pl.par : (pl.par < 0 || dup_rows || n < 2048 ? 0 : 16));
        parg = std::min(std::min(parg, WIDE_PAR_GMAX), xcd_cus);
        if (parg == 1) parg = 0;
        if (parg > 1) {
            if (g_par_busy[device_slot].exchange(1) != 0) parg = 0;
            else par_slot.p = &g_par_busy[device_slot];
        }
        const size_t parb = parg > 0 ? wide_par_state_bytes(n, parg) : 0;
        const size_t sc_off = ((2 * nT + 255) / 256) * 256;            // the phase machine's control block behind everything else
        const size_t par_off = sc_off + WIDE_SC_BYTES;
        const size_t scx_off = ((par_off + parb + 255) / 256) * 256;     // the machine's own arrays (scx_off_*)
        // the embedded form of the searches (wide_aug<.., EMB>): several searches at once with the prices in global memory
        // (developer knob, read once per process: CYTO_AUG_EMBED = 1 or unset: where the longest inverse list allows; 0: never; 2: always)
        bool vlds_k, clds_k;
        wide_aug_lds_choice(n, vlds_k, clds_k);
        const bool emb_cand = parg > 1 && !vlds_k && n <= (1 << 25) && embed_knob != 0;
        const size_t emb_off = ((scx_off + wide_sc_ext_bytes(n) + 255) / 256) * 256;
        if ((rc = j.state->alloc(emb_cand ? emb_off + wide_embed_bytes(n) : scx_off + wide_sc_ext_bytes(n), stream))) return rc;
        WideArgs &wa = h_wa[(size_t)k];
        wa.cache_red = nullptr; wa.inv_off = nullptr; wa.inv_ent = nullptr; wa.emb_longest = nullptr;
        if (emb_cand) {
            char *eb = j.state->as<char>() + emb_off;
            wa.cache_red = reinterpret_cast<float *>(eb);
            wa.inv_off = reinterpret_cast<int32_t *>(eb + emb_off_inv(n));
            wa.inv_ent = reinterpret_cast<unsigned long long *>(eb + emb_off_ent(n));
            if (embed_knob == 1) wa.emb_longest = emb_counts(wa, n) + n;        // (the gate: both forms are enqueued, the device chooses)
        }
        wa.n = n; wa.ld = j.ld; wa.cost = j.cost; wa.rowmap = j.rowmap;
        wa.v = j.fws + FWS_V * (int64_t)n; wa.u = j.fws + FWS_U * (int64_t)n; wa.cassign = j.fws + FWS_CASSIGN * (int64_t)n;
        wa.label = reinterpret_cast<unsigned long long *>(j.fws + FWS_LABEL * (int64_t)n);
        wa.rowsol = j.iws + IWS_ROWSOL * (int64_t)n; wa.colsol = j.iws + IWS_COLSOL * (int64_t)n; wa.matches = j.iws + IWS_MATCHES * (int64_t)n;
        wa.freerows = j.iws + IWS_FREEROWS * (int64_t)n;
        wa.act0 = j.iws + IWS_ACT0 * (int64_t)n; wa.act1 = j.iws + IWS_ACT1 * (int64_t)n; wa.touched = j.iws + IWS_TOUCHED * (int64_t)n;
        wa.slot_j = j.iws + IWS_SLOT_J * (int64_t)n;
        wa.bid = reinterpret_cast<unsigned long long *>(j.iws + IWS_BID * (int64_t)n);
        wa.slot_p = j.state->as<float>(); wa.slot_c = wa.slot_p + n;
        wa.cache_col = j.cache_col; wa.cache_val = j.cache_val; wa.misc = j.misc;
        wa.max_rounds = pl.rounds;
        wa.aug_seg = pl.rebuild;
        // what a rebuild costs, in full-row relaxations of ONE workgroup (a relaxation sweeps n elements at ~5 G/s; a pass costs
        // ~0.4 ms of launches and synchronisation plus one read of every unfinished problem's matrix by the whole chip, ~100x
        // faster per element -- and the problems of a batch are rebuilt one after the other while their workgroups all wait)
        wa.aug_waste = (int)std::min<long long>(1 << 30, std::max<long long>(16, (2000000ll + (long long)nl * n * n / 100) / n));
        wa.arr_waste = std::max(8, wa.aug_waste / 3);          // (a full-row bid with its cache refresh: three sweeps)
        if (CYTO_KNOB("CYTO_ARR_WASTE").set) wa.arr_waste = std::max(1, CYTO_KNOB("CYTO_ARR_WASTE").value);     // (developer knob, read once per process: tools/batch_chunks_bench.py)
        wa.seg_quorum = nl > 1 ? std::max(1, nl / 4) : 0;
        wa.seg_sync = nullptr;
        wa.same_prev = j.same;
        wa.sc = j.state->as<char>() + sc_off;
        CYTO_HIP(hipMemsetAsync(wa.sc, 0, WIDE_SC_BYTES, stream));
        wa.scx = j.state->as<char>() + scx_off;
        CYTO_HIP(hipMemsetAsync(wa.scx, 0, wide_sc_ext_bytes(n), stream));
        CYTO_HIP(hipMemsetAsync(wa.scx, 0xFF, wide_sc_ones_bytes(n), stream));     // (the machine's bid words and lowest-bid arrays)
        wa.par_groups = parg; wa.par = nullptr;
        // (developer knob, read once per process: CYTO_AUG_ABORT = 1 or unset: searches that can no longer be committed end early; 0: they
        //  run to their ends -- same batches, same results: tests/test_wide_abort_gpu.py, the A/B of profiles/r11_doomed_ab.txt)
        wa.aug_abort = CYTO_KNOB("CYTO_AUG_ABORT").set ? (CYTO_KNOB("CYTO_AUG_ABORT").value != 0 ? 1 : 0) : 1;
        if (parg > 0) {
            wa.par = j.state->as<char>() + par_off;
            if (!par_view_ok(wa)) return CYTO_ERR_INTERNAL;                                                   // (the kernels' view of the state and the offsets used here: one layout)
            CYTO_HIP(hipMemsetAsync(wa.par, 0, PAR_CTL_BYTES, stream));                                        // the control block ...
            // ... P[0], P[1]: "no conflict"  (a fill, not a copy from a local: a copy had the host wait here, through the column pass,
            //  and what follows -- memsets, wide_rt, the first round launches -- was enqueued onto an idle chip)
            CYTO_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(wa.par + offsetof(ParCtl, P)), WIDE_PAR_GMAX + 1, 2, stream));
            CYTO_HIP(hipMemsetAsync(wa.par + par_off_labels(n, parg), 0xFF, par_off_touched(n, parg) - par_off_labels(n, parg), stream));     // every search's labels: all-ones
            CYTO_HIP(hipMemsetAsync(wa.par + par_off_claim(n, parg), 0, par_off_plog_col(n, parg) - par_off_claim(n, parg), stream));       // the claim words
        }
        // the post-column-reduction prices: snapshot for the reduction transfer AND the raw cost of every owner entry
        CYTO_HIP(hipMemcpyAsync(wa.cassign, wa.v, nT, hipMemcpyDeviceToDevice, stream));
        CYTO_HIP(hipMemsetAsync(wa.label, 0xFF, 2 * nT, stream));
        CYTO_HIP(hipMemsetAsync(wa.bid, 0xFF, 2 * nT, stream));
    }
    DevBuf d_wa, d_sync;
    if ((rc = d_wa.alloc(sizeof(WideArgs) * nl, stream)) || (rc = d_sync.alloc(sizeof(int32_t) * ((size_t)nl + 1), stream))) return rc;
    for (WideArgs &wa : h_wa) wa.seg_sync = d_sync.as<int32_t>();
    CYTO_HIP(hipMemcpyAsync(d_wa.p, h_wa.data(), sizeof(WideArgs) * nl, hipMemcpyHostToDevice, stream));
    if ((rc = wide_launch_rt(d_wa.as<WideArgs>(), nl, n, stream))) return rc;
    std::vector<int32_t> h_sync((size_t)nl + 1, 1);
    std::vector<int32_t> caches_fresh((size_t)nl, 0);           // (wide_arr's word: hardly a full-row bid -- no rebuild before the searches)
    using BuildFn = decltype(build_caches_of);
    auto rebuild_tramp = +[](void *ctx, const int32_t *flags) -> int { return (*static_cast<BuildFn *>(ctx))(flags); };
    for (int pass = 0;; pass++) {                              // the row-reduction rounds (they pause when the caches have gone stale)
        if (pass && (rc = build_caches_of(h_sync.data() + 1))) return rc;
        CYTO_HIP(hipMemsetAsync(d_sync.p, 0, sizeof(int32_t), stream));
        if ((rc = wide_launch_arr(d_wa.as<WideArgs>(), nl, n, stream, pl.wipe, pass > 0, d_sync.as<int32_t>(), rebuild_tramp, &build_caches_of,
                                  nl == 1 ? &h_wa[0] : nullptr))) return rc;
        if (h_wa[0].aug_seg != 0) break;                       // (no pauses asked for: nothing to wait for)
        CYTO_HIP(hipMemcpyAsync(h_sync.data(), d_sync.p, sizeof(int32_t) * ((size_t)nl + 1), hipMemcpyDeviceToHost, stream));
        CYTO_HIP(hipStreamSynchronize(stream));
        bool done = true;
        for (int k = 0; k < nl; k++) { done = done && (h_sync[(size_t)k + 1] & 1) == 0; caches_fresh[(size_t)k] = (h_sync[(size_t)k + 1] & 2) != 0; h_sync[(size_t)k + 1] &= 1; }
        if (done) break;
    }
    // the searches, in as many launches as they ask for: wide_aug returns when its row caches have gone stale and the whole chip
    // rebuilds them against the prices reached -- only for the problems that still have searches to run
    const int parg = h_wa[0].par_groups;
    for (int pass = 0;; pass++) {
        if (pass == 0) {
            std::vector<int32_t> need((size_t)nl);
            for (int k = 0; k < nl; k++) need[(size_t)k] = caches_fresh[(size_t)k] ? 0 : 1;
            if ((rc = build_caches_of(need.data()))) return rc;
        } else if ((rc = build_caches_of(h_sync.data() + 1))) return rc;
        if (pass == 0) CYTO_HIP(hipEventRecord(ev_arr_done, stream));   // (ms_aug: the search kernel -- and what later passes add)
        if (pass == 0 && parg == 0) {
            // repeated spot rows (CytoSPACE's slots): their one-edge searches all at once, before the search kernel
            bool dup = false;
            for (int k = 0; k < nl; k++) dup = dup || h_wa[(size_t)k].same_prev != nullptr;
            if (dup && (rc = wide_launch_claims(d_wa.as<WideArgs>(), nl, n, stream, d_sync.as<int32_t>()))) return rc;
        }
        bool embed = false;
        if (parg > 0 && h_wa[0].cache_red) {                   // (one launch runs all searches: the caches are not rebuilt behind this)
            if ((rc = wide_build_embedded(h_wa[0], n, stream))) return rc;
            embed = true;                                      // (knob 2: always; knob 1: where the gate allows -- wide_aug reads it)
        }
        CYTO_HIP(hipMemsetAsync(d_sync.p, 0, sizeof(int32_t), stream));
        if ((rc = wide_launch_aug(d_wa.as<WideArgs>(), nl, n, stream, parg, embed))) return rc;
        // the gate (emb_longest): the plain twin right behind the embedded kernel, and one of the two returns at once.  Which one ran
        // comes back in the status block (LapStatus::wide_embedded: wide_note_status)
        if (embed && h_wa[0].emb_longest && (rc = wide_launch_aug(d_wa.as<WideArgs>(), nl, n, stream, parg, false))) return rc;
        if (parg > 0) { CYTO_HIP(hipStreamSynchronize(stream)); break; }    // (the slot of g_par_busy is held until both have drained)
        CYTO_HIP(hipMemcpyAsync(h_sync.data(), d_sync.p, sizeof(int32_t) * ((size_t)nl + 1), hipMemcpyDeviceToHost, stream));
        CYTO_HIP(hipStreamSynchronize(stream));                // (d_wa is read by the kernels until here)
        bool done = true;
        for (int k = 0; k < nl; k++) done = done && h_sync[(size_t)k + 1] == 0;
        if (done) break;
    }
    return CYTO_OK;
}

void wide_note_status(const LapStatus &h) {
    if (h.wide_embedded) g_embedded_solves.fetch_add(1);
    if (h.wide_aborted > 0) g_aborted_searches.fetch_add(h.wide_aborted);
}

void wide_info(cyto_lap_info *info, const LapStatus &h) {
    const long long *wc = h.wide, *tm = h.timers;       // (timers: diagnostics for tools/wide_large.py; 100 MHz ticks)
    info->wide = 1;
    info->aug_handover = -1;                            // (the chain solver's: no hand-over)
    info->wide_rounds = wc[WC_ROUNDS]; info->wide_retired = wc[WC_RETIRED]; info->wide_dense_arr = wc[WC_DENSE_ARR];
    info->wide_dense_aug = wc[WC_DENSE_AUG]; info->wide_aug_rounds = wc[WC_AUG_ROUNDS]; info->wide_aug_settled = wc[WC_AUG_PROCESSED];
    info->wide_trivial = wc[WC_TRIVIAL]; info->wide_verify_passes = wc[WC_VERIFY_PASSES]; info->wide_aug_launches = wc[WC_AUG_LAUNCHES];
    info->wide_list_rounds = tm[WT_LIST_ROUNDS]; info->wide_chain_rounds = tm[WT_CHAIN_ROUNDS];
    info->wide_ms_list = tm[WT_LIST_TICKS] * 1e-5; info->wide_ms_chain = tm[WT_CHAIN_TICKS] * 1e-5;
    info->wide_ms_aug_rounds = tm[WT_AUG_ROUNDS_TICKS] * 1e-5; info->wide_ms_aug_verify = tm[WT_AUG_VERIFY_TICKS] * 1e-5;
    info->wide_ms_aug_finish = tm[WT_AUG_FINISH_TICKS] * 1e-5; info->wide_ms_aug_trivial = tm[WT_AUG_TRIVIAL_TICKS] * 1e-5;
    info->wide_arr_launches = tm[WT_ARR_LAUNCHES]; info->wide_scaled = tm[WT_SCALED]; info->wide_phases = tm[WT_PHASES];
    info->wide_par_batches = tm[WT_PAR_BATCHES]; info->wide_par_discarded = tm[WT_PAR_DISCARDED];
}

}  // namespace cyto

extern "C" long long cyto_wide_embedded_solves(void) { return cyto::g_embedded_solves.load(); }
extern "C" long long cyto_wide_aborted_searches(void) { return cyto::g_aborted_searches.load(); }
