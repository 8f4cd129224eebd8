// Batch pipeline: HBM-resident batch object, kernel wrappers and the batch-level C ABI.
// (included by rtk_device.hip)
#include "rtk_seeds.h"
#include "rtk_region.h"
#include "rtk_region_enum.h"
#include "rtk_region_lane.h"
#ifdef RTK_SIM
thread_local RlEnv rl_env; thread_local uint32_t rl_lst[RL_S_N * RL_STRIDE]; thread_local uint64_t rl_peq_all[RL_NSYM * RL_MAXW * RL_STRIDE];
#endif
#include "rtk_phasing.h"
#include "rtk_fixsnps.h"
#ifndef RTK_SIM
#include "rtk_phase_long.h"
#endif

// ------------------------------------------------------------------------------------------------ kernels
// the views of the next launches of a batch, written once where every wave reads them (rtk_region_types.h: LaunchCtx)
RTK_GLOBAL void k_set_ctx(LaunchCtx* out, GraphView g, OptsView o, BatchView bv, RegionBatch rb) {
    if (RTK_BLOCK_ID == 0 && rtk_lane() == 0) { out->g = g; out->o = o; out->bv = bv; out->rb = rb; }
}

// ------------------------------------------------------------------------------------------------ batch object
struct rtk_batch {
    rtk_graph* g = nullptr;
    uint32_t n = 0; uint64_t n_bases = 0;
    std::vector<uint64_t> roff;
    std::vector<std::pair<void*, uint64_t> > owned; // device allocations (pointer, bytes), returned to the graph's pool
    BatchView bv;
    rtk_stats stats;
    // region stage
    RegionBatch rb;
    bool seeded = false, ran = false;
    rtk_stream_t stream = 0; bool has_stream = false;
    void (*on_region_slab)(void*) = nullptr; void* on_region_slab_arg = nullptr; // called once when the region stage of this batch has its work areas (the ticket coalescing of rtk_correct_batch paces its groups by it)
    rtk_stream_t stream2 = 0; bool has_stream2 = false; rtk_event_t ev[2]; // second stream of the region stage (the lane kernel beside the wave kernel) and the two events that order it
    rtk_stream_t lane_stream() { if (!has_stream2) { stream2 = rtk_stream_create_high(); ev[0] = rtk_event_create(); ev[1] = rtk_event_create(); has_stream2 = true; } return stream2; }
    RtkTimer t_all;
    // host side of rtk_batch_fetch_view: the packed records in pinned staging memory + their offsets / lengths
    void* h_out = nullptr; uint64_t h_out_bytes = 0; std::vector<uint64_t> h_off; std::vector<uint32_t> h_sl, h_ql;
    // second pass: the uncorrected reads (phasing() re-reads them, src/Ratatosk.cpp:774-802,832) and whether the pre-filter has run
    char* d_raw = nullptr; uint64_t* d_raw_off = nullptr; uint64_t raw_bases = 0; uint32_t raw_max_len = 0; bool has_raw = false, phased = false, snps_fixed = false;
    uint64_t* d_mask_items = nullptr; uint32_t n_mask_items = 0, mask_seg = 0; // work list of k_mask (first pass): segments of mask_seg windows
    LaunchCtx* d_ctx = nullptr; // the views of the launches of this batch (k_set_ctx)
    LaunchCtx* ctx() { if (!d_ctx) d_ctx = alloc<LaunchCtx>(1); return d_ctx; }
    void alloc_arrays() { // everything sized by the number of bases / reads of the batch as it stands (again after the phasing step changed the reads)
        bv.hits = alloc<uint64_t>(n_bases + 64);
        bv.hitmap = alloc<uint64_t>(n_bases / 64 + 4);
        bv.masked = alloc<char>(n_bases + 64);
        bv.wdesc = alloc<uint64_t>(n_bases + 64);
        bv.ipool_cap = std::max<uint64_t>(4096, n_bases / 2) + 4096ull * 4096ull; // + one private chunk per resident wave
        bv.ipool = alloc<uint64_t>(2 * bv.ipool_cap);
        bv.ipool_top = alloc<unsigned long long>(1);
        bv.s_pos = alloc<uint32_t>(n_bases + 64); bv.n_solid = alloc<uint32_t>(n);
        bv.wk_cap = std::max<uint64_t>(4096, n_bases / 2); bv.wk_pos = alloc<uint32_t>(bv.wk_cap); bv.wk_hit = alloc<uint64_t>(bv.wk_cap); bv.wk_top = alloc<unsigned long long>(1);
        bv.w_off = alloc<uint64_t>(n); bv.w_cnt = alloc<uint32_t>(n);
        bv.status = alloc<uint32_t>(n); bv.counters = alloc<unsigned long long>(RTK_CNT_TOTAL);
    }
    rtk_batch() { memset(&bv, 0, sizeof(bv)); memset(&stats, 0, sizeof(stats)); memset(&rb, 0, sizeof(rb)); }
    // A batch takes ONE buffer from the graph's pool, sized for everything it will ask for (rtk_batch_arena_bytes), and carves its ~45 arrays out of it; what does not
    // fit (a second set of arrays after the phasing step, grown capacities) comes from the pool one by one as before. One pool request per ticket instead of 45 -- and a miss costs
    // ONE hipMalloc, which rtk_graph_reserve_batches lets a caller pay before the correction phase (a hipMalloc stalls every stream of the device: 0.15-2.1 s per second-pass run
    // of 5.7 s went into ~165 of them, profiles/r06_pass2_trace.txt).
    char* arena = nullptr; uint64_t arena_bytes = 0, arena_top = 0;
    void arena_reserve(uint64_t bytes) { if (arena || !bytes) return; uint64_t got = 0; arena = static_cast<char*>(g->pool_take(bytes, &got)); owned.push_back(std::make_pair(static_cast<void*>(arena), got)); arena_bytes = got; arena_top = 0; }
    template <class T> T* alloc(uint64_t count) {
        const uint64_t bytes = (sizeof(T) * (count ? count : 1) + 255ull) & ~255ull;
        if (arena && arena_top + bytes <= arena_bytes) { T* p = reinterpret_cast<T*>(arena + arena_top); arena_top += bytes; return p; }
        uint64_t got = 0; void* p = g->pool_take(bytes, &got); owned.push_back(std::make_pair(p, got)); return static_cast<T*>(p);
    }
    ~rtk_batch() { if (has_stream2) { try { rtk_ssync(stream2); } catch (...) {} rtk_stream_destroy(stream2); rtk_event_destroy(ev[0]); rtk_event_destroy(ev[1]); } if (has_stream) { try { rtk_ssync(stream); } catch (...) {} rtk_stream_destroy(stream); } if (g) { if (h_out) g->stage_give(h_out, h_out_bytes); for (size_t i = 0; i < owned.size(); ++i) g->pool_give(owned[i].first, owned[i].second); graph_release(g); } }
};

static bool opts_ok(const rtk_opts* o) { return o->struct_size == static_cast<uint32_t>(sizeof(rtk_opts)); }
static OptsView opts_view(const rtk_opts* o) {
    OptsView v;
    v.insert_sz = static_cast<uint32_t>(o->insert_sz); v.min_cov_vertices = static_cast<uint32_t>(o->min_cov_vertices);
    v.max_len_weak_region1 = static_cast<uint32_t>(o->max_len_weak_region1); v.max_km_cov = static_cast<uint32_t>(o->max_km_cov > 0xFFFFFFFFull ? 0xFFFFFFFFull : o->max_km_cov);
    v.weak_region_len_factor = o->weak_region_len_factor; v.large_k_factor = o->large_k_factor; v.min_score = o->min_score; v.max_qual = o->max_qual; v.out_qual = o->out_qual; v.min_confidence_snp_corr = o->min_confidence_snp_corr;
    v.a2_exclusive = (o->a2_exclusive == 2) ? 2u : (o->a2_exclusive ? 1u : 0u); v.a3_strand_order = o->a3_strand_order ? 1u : 0u; v.d1_desc = o->d1_desc ? 1u : 0u;
    v.fa_linked_always = rtk_knob_fa_linked_always() ? 1u : 0u; // (a knob, not an option: it cannot change a result)
    v.strand2_mode = rtk_knob_strand2_always() ? 1u : (rtk_knob_strand2_audit() ? 2u : 0u); // (knobs as well: the bytes are the same under all three)
    v.colours_mode = rtk_knob_colours_route() | (rtk_knob_colours_audit() << 2); // RTK_CM_* (the selection is the same under every setting)
    v.park_eager = rtk_knob_park_eager() ? 1u : 0u;
    v.trim_store = rtk_knob_trim_store() ? 1u : 0u;
    v.inexact_route = (rtk_knob_inexact_shared() ? 0u : RTK_IR_PER_WINDOW) | (rtk_knob_inexact_planes() ? 0u : RTK_IR_TEXT_PACK);
    v.long_read_correct = o->long_read_correct ? 1 : 0; v.max_len_weak_region2 = static_cast<uint32_t>(o->max_len_weak_region2 > 0xFFFFFFFFull ? 0xFFFFFFFFull : o->max_len_weak_region2);
    return v;
}

// k_mask cuts the reads into segments of this many windows, one wave each (a multiple of 64 windows x the lanes of a wave; RTK_MASK_SEG: tests)
static uint32_t mask_seg() { const uint32_t unit = 64u * RTK_WAVE; uint32_t v = rtk_knob_mask_seg(); v = (v + unit - 1) / unit * unit; return v ? v : unit; }

// what a batch of n reads / n_bases bases asks the pool for over its life (first pass: staging copy, seed-stage arrays, region arrays, segment and output pools; the raw-hit
// pool holds one private chunk per resident wave: 268 MB whatever the ticket): ~62 B per base + 400 B per read + 280 MB, rounded up generously -- a short arena only means
// a few single requests
static uint64_t rtk_batch_arena_bytes(uint64_t n_bases, uint64_t n, bool with_qual, uint64_t raw_bases) {
    return 66ull * n_bases + (with_qual ? 2ull * n_bases : 0ull) + 2ull * raw_bases + 640ull * n + (300ull << 20);
}
static thread_local uint64_t t_arena_extra = 0; // rtk_batch_create2 -> rtk_batch_create: the second pass asks for more (the uncorrected reads, the arrays a second time after the phasing step)
static uint64_t rtk_second_pass_extra(uint64_t n_bases, uint64_t raw_bases) { return 42ull * n_bases + 2ull * raw_bases + (64ull << 20); }
extern "C" int rtk_graph_reserve_batches(rtk_graph* g, uint32_t n_batches, uint64_t bases_per_batch, uint32_t reads_per_batch, int with_qualities, uint64_t raw_bases_per_batch) {
    if (!g) return rtk_fail(RTK_ERR_ARG, "rtk_graph_reserve_batches: null argument");
    if (!g->on_device) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_graph_reserve_batches: graph is not resident on a device");
#ifdef RTK_SIM
    (void)n_batches; (void)bases_per_batch; (void)reads_per_batch; (void)with_qualities; (void)raw_bases_per_batch; return RTK_OK;
#else
    std::vector<std::pair<void*, uint64_t> > held; int rc = RTK_OK;
    try {
        rtk_set_device(g->device);
        const uint64_t want = rtk_batch_arena_bytes(bases_per_batch, reads_per_batch, with_qualities != 0, 0) + (raw_bases_per_batch ? rtk_second_pass_extra(bases_per_batch, raw_bases_per_batch) : 0ull);
        // all of them are TAKEN before any is given back: the pool serves a request from the first parked buffer that is big enough, so taking and parking one at a time would
        // find the same buffer n times
        for (uint32_t i = 0; i < n_batches; ++i) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || static_cast<uint64_t>(fr) < want + static_cast<uint64_t>(tot) / 8) { rc = rtk_fail(RTK_ERR_DEVICE, "rtk_graph_reserve_batches: not all reserved (less than an eighth of the device memory would stay free)"); break; }
            uint64_t got = 0; void* p = g->pool_take(want, &got); held.push_back(std::make_pair(p, got));
        }
    } catch (const std::exception& e) { rc = rtk_fail(RTK_ERR_DEVICE, std::string("rtk_graph_reserve_batches: ") + e.what()); }
    for (size_t j = 0; j < held.size(); ++j) g->pool_give(held[j].first, held[j].second);
    // the pinned staging buffers of the same tickets (packed reads in, packed records out, the uncorrected reads of the second pass): a hipHostMalloc of 67 MB keeps its worker
    // thread for ~20 ms (8 calls, 130-220 ms per second-pass run before this)
    try {
        std::vector<std::pair<void*, uint64_t> > hh;
        const uint64_t in_b = bases_per_batch * (with_qualities ? 2ull : 1ull) + 16ull * reads_per_batch + (1ull << 16), out_b = 2ull * (bases_per_batch + bases_per_batch / 8) + 8;
        for (uint32_t i = 0; i < n_batches; ++i) {
            uint64_t got = 0; void* p = g->stage_take(in_b, &got); hh.push_back(std::make_pair(p, got));
            p = g->stage_take(out_b, &got); hh.push_back(std::make_pair(p, got));
            if (raw_bases_per_batch) { p = g->stage_take(raw_bases_per_batch + 64, &got); hh.push_back(std::make_pair(p, got)); }
        }
        for (size_t j = 0; j < hh.size(); ++j) g->stage_give(hh[j].first, hh[j].second);
    } catch (const std::exception& e) { if (rc == RTK_OK) rc = rtk_fail(RTK_ERR_DEVICE, std::string("rtk_graph_reserve_batches: ") + e.what()); }
    return rc;
#endif
}

extern "C" int rtk_batch_create(rtk_graph* g, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len, rtk_batch** out) {
    // pass 1 replaces every quality (src/Correction.cpp:184-185; the clamp of src/Ratatosk.cpp:816 has no observable effect); pass 2 carries
    // them over, so they travel with the reads when the caller has them
    if (!g || !seq || !len || !out) return rtk_fail(RTK_ERR_ARG, "rtk_batch_create: null argument");
    bool have_qual = qual != nullptr;
    for (uint32_t i = 0; have_qual && i < n; ++i) have_qual = qual[i] != nullptr || len[i] == 0;
    if (!g->on_device) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_batch_create: graph is not resident on a device (call rtk_graph_upload); there is no CPU fallback");
    try {
        rtk_set_device(g->device);
        std::unique_ptr<rtk_batch> b(new rtk_batch());
        b->g = g; b->n = n; g->refs.fetch_add(1);
        b->stream = rtk_stream_create(); b->has_stream = true;
        b->roff.assign(n + 1, 0);
        for (uint32_t i = 0; i < n; ++i) b->roff[i + 1] = b->roff[i] + len[i];
        b->n_bases = b->roff[n];
        b->arena_reserve(rtk_batch_arena_bytes(b->n_bases, n, have_qual, 0) + t_arena_extra);
        // the reads are packed (upper-cased: src/Ratatosk.cpp:814) into pinned staging memory, next to their offsets and the
        // longest-first order, and go to the device with ONE asynchronous copy on the batch's stream
        const uint64_t seq_bytes = (b->n_bases + 64 + 7) / 8 * 8, roff_bytes = 8ull * (n + 1), ord_bytes = (4ull * n + 7) / 8 * 8, qual_bytes = have_qual ? seq_bytes : 0;
        uint64_t stage_bytes = 0;
        char* stage = static_cast<char*>(g->stage_take(seq_bytes + roff_bytes + ord_bytes + qual_bytes, &stage_bytes));
        struct StageGuard { rtk_graph* g; void* p; uint64_t n; ~StageGuard() { g->stage_give(p, n); } } guard = {g, stage, stage_bytes};
        // (reads of a ticket are packed by up to four threads: one thread moves ~2 GB/s out of buffers another core has just parsed, a ticket is 30-130 MB)
        char* const qs = have_qual ? stage + seq_bytes + roff_bytes + ord_bytes : nullptr;
        auto pack_range = [&](uint32_t lo, uint32_t hi) {
            for (uint32_t i = lo; i < hi; ++i) {
                const unsigned char* __restrict__ src = reinterpret_cast<const unsigned char*>(seq[i]); unsigned char* __restrict__ dst = reinterpret_cast<unsigned char*>(stage) + b->roff[i];
                const uint32_t l = len[i];
                for (uint32_t j = 0; j < l; ++j) { const unsigned char ch = src[j]; dst[j] = static_cast<unsigned char>(ch - ((static_cast<unsigned char>(ch - 'a') < 26u) ? 32u : 0u)); }
                if (qs && l) memcpy(qs + b->roff[i], qual[i], l);
            }
        };
        {
            const uint32_t n_thr = (b->n_bases >= (4u << 20) && n >= 8) ? 4u : 1u;
            std::vector<uint32_t> cut(n_thr + 1, n); cut[0] = 0;
            for (uint32_t t = 1, i = 0; t < n_thr; ++t) { const uint64_t want = b->n_bases / n_thr * t; while (i < n && b->roff[i] < want) ++i; cut[t] = i; }
            std::vector<std::thread> thr;
            for (uint32_t t = 1; t < n_thr; ++t) thr.emplace_back(pack_range, cut[t], cut[t + 1]);
            pack_range(cut[0], cut[1]);
            for (size_t t = 0; t < thr.size(); ++t) thr[t].join();
        }
        memset(stage + b->n_bases, 'N', seq_bytes - b->n_bases);
        memcpy(stage + seq_bytes, b->roff.data(), roff_bytes);
        { uint32_t* ord = reinterpret_cast<uint32_t*>(stage + seq_bytes + roff_bytes); for (uint32_t i = 0; i < n; ++i) ord[i] = i;
          std::stable_sort(ord, ord + n, [&](uint32_t x, uint32_t y) { return len[x] > len[y]; }); }
        BatchView& bv = b->bv;
        bv.n_reads = n; bv.n_bases = b->n_bases;
        if (have_qual) memset(qs + b->n_bases, '!', qual_bytes - b->n_bases);
        char* dstage = b->alloc<char>(seq_bytes + roff_bytes + ord_bytes + qual_bytes);
        rtk_h2d_s(dstage, stage, seq_bytes + roff_bytes + ord_bytes + qual_bytes, b->stream);
        bv.qual = have_qual ? dstage + seq_bytes + roff_bytes + ord_bytes : nullptr;
        bv.seq = dstage; bv.roff = reinterpret_cast<uint64_t*>(dstage + seq_bytes); bv.order = reinterpret_cast<uint32_t*>(dstage + seq_bytes + roff_bytes);
        b->alloc_arrays();
        std::vector<uint64_t> items; // work list of k_mask: the reads in longest-first order, cut into segments of mask_seg() windows
        b->mask_seg = mask_seg();
        { const uint32_t* ord = reinterpret_cast<const uint32_t*>(stage + seq_bytes + roff_bytes); const uint32_t kk = static_cast<uint32_t>(g->dview.k);
          for (uint32_t i = 0; i < n; ++i) { const uint32_t r = ord[i], l = len[r]; if (l <= kk) continue; const uint32_t nwin = l - kk + 1, ns = (nwin + b->mask_seg - 1) / b->mask_seg; for (uint32_t sg = 0; sg < ns; ++sg) items.push_back((static_cast<uint64_t>(r) << 32) | sg); }
          b->n_mask_items = static_cast<uint32_t>(items.size()); b->d_mask_items = b->alloc<uint64_t>(items.size()); rtk_h2d_s(b->d_mask_items, items.data(), 8ull * items.size(), b->stream); }
        rtk_ssync(b->stream); // the staging buffer goes back to the pool
        *out = b.release();
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return RTK_OK;
}

#include "rtk_seed_stage.inc"

// The one reader of the seed stage's output layout (BatchView, rtk_seed_types.h): the anchors of read `read` of a batch whose seed stage has completed, as
// (pos, unitig, dist, strand) quadruples with positions in the read's own coordinates. Read r keeps its solid positions at s_pos[roff[r] .. + n_solid[r])
// and looks their hits up in hits[roff[r] + pos]; its weak anchors are wk_pos / wk_hit[w_off[r] .. + w_cnt[r]). Up to `cap` quadruples of each list are
// written; the counts are always the true ones, and a list longer than `cap` is an RTK_ERR_ARG in the name of the entry `who`.
static int read_anchors(rtk_batch* b, uint32_t read, uint64_t* n_solid, int64_t* solid, uint64_t* n_weak, int64_t* weak, uint64_t cap, const char* who) {
    const uint64_t base = b->roff[read]; const uint64_t len = b->roff[read + 1] - base;
    uint32_t ns = 0, nw = 0; uint64_t woff = 0;
    rtk_d2h(&ns, b->bv.n_solid + read, 4); rtk_d2h(&nw, b->bv.w_cnt + read, 4); rtk_d2h(&woff, b->bv.w_off + read, 8);
    std::vector<uint32_t> sp(ns + 1), wp(nw + 1); std::vector<uint64_t> hits(len + 1), wh(nw + 1);
    rtk_d2h(sp.data(), b->bv.s_pos + base, 4ull * ns); rtk_d2h(hits.data(), b->bv.hits + base, 8ull * len);
    rtk_d2h(wp.data(), b->bv.wk_pos + woff, 4ull * nw); rtk_d2h(wh.data(), b->bv.wk_hit + woff, 8ull * nw);
    *n_solid = ns; *n_weak = nw;
    for (uint32_t i = 0; i < ns && i < cap; ++i) { const UMap u = rtk_unpack_hit(hits[sp[i]]); solid[4 * i] = sp[i]; solid[4 * i + 1] = u.unitig; solid[4 * i + 2] = u.dist; solid[4 * i + 3] = u.strand; }
    for (uint32_t i = 0; i < nw && i < cap; ++i) { const UMap u = rtk_unpack_hit(wh[i]); weak[4 * i] = wp[i]; weak[4 * i + 1] = u.unitig; weak[4 * i + 2] = u.dist; weak[4 * i + 3] = u.strand; }
    if (ns > cap || nw > cap) return rtk_fail(RTK_ERR_ARG, std::string(who) + ": output capacity too small");
    return RTK_OK;
}

extern "C" int rtk_seeds(rtk_graph* g, const rtk_opts* opts, const char* seq, uint32_t len, uint64_t* n_solid, int64_t* solid, uint64_t* n_weak, int64_t* weak, uint64_t cap) {
    if (!g || !opts || !seq || !n_solid || !solid || !n_weak || !weak) return rtk_fail(RTK_ERR_ARG, "rtk_seeds: null argument");
    if (!opts_ok(opts)) return rtk_fail(RTK_ERR_ARG, "rtk_seeds: rtk_opts was not filled by this library's rtk_opts_default (struct_size does not match: older header, or a zero-filled struct)");
    rtk_batch* b = nullptr;
    const char* seqs[1] = {seq}; const uint32_t lens[1] = {len};
    int rc = rtk_batch_create(g, 1, seqs, nullptr, lens, &b);
    if (rc) return rc;
    try {
        rc = seed_stage_checked(b, opts_view(opts));
        if (rc == RTK_OK) rc = read_anchors(b, 0, n_solid, solid, n_weak, weak, cap, "rtk_seeds");
    } catch (const std::exception& e) { rc = rtk_fail(RTK_ERR_DEVICE, e.what()); }
    delete b;
    return rc;
}

extern "C" int rtk_batch_fetch_seeds(rtk_batch* b, uint32_t read, uint64_t* n_solid, int64_t* solid, uint64_t* n_weak, int64_t* weak, uint64_t cap) {
    if (!b || !n_solid || !solid || !n_weak || !weak) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch_seeds: null argument");
    if (!b->seeded) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch_seeds: rtk_batch_run_seeds has not completed for this batch (or its region stage has run since)");
    if (read >= b->n) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch_seeds: the batch has no such read");
    try {
        rtk_set_device(b->g->device);
        return read_anchors(b, read, n_solid, solid, n_weak, weak, cap, "rtk_batch_fetch_seeds");
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
}

extern "C" void rtk_batch_free(rtk_batch* b) { delete b; }


// ------------------------------------------------------------------------------------------------ second pass: phasing pre-filter
// rtk_batch_create + the uncorrected reads in the same order (reference: the raw / corrected lock-step reader, src/Ratatosk.cpp:774-802).
extern "C" int rtk_batch_create2(rtk_graph* g, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len,
                                 const char* const* raw, const uint32_t* raw_len, rtk_batch** out) {
    if (!raw || !raw_len || !qual) return rtk_fail(RTK_ERR_ARG, "rtk_batch_create2: the second pass needs qualities and the uncorrected reads");
    if (!len) return rtk_fail(RTK_ERR_ARG, "rtk_batch_create2: null argument");
    { uint64_t nb = 0, rbs = 0; for (uint32_t i = 0; i < n; ++i) { nb += len[i]; rbs += raw_len[i]; } t_arena_extra = rtk_second_pass_extra(nb, rbs); }
    int rc = rtk_batch_create(g, n, seq, qual, len, out);
    t_arena_extra = 0;
    if (rc) return rc;
    rtk_batch* b = *out;
    try {
        std::vector<uint64_t> ro(n + 1, 0);
        for (uint32_t i = 0; i < n; ++i) { ro[i + 1] = ro[i] + raw_len[i]; b->raw_max_len = std::max(b->raw_max_len, raw_len[i]); }
        b->raw_bases = ro[n];
        // packed into pinned staging memory by up to four threads, like the corrected reads (as read from the file: not upper-cased, src/Ratatosk.cpp:781)
        uint64_t stage_bytes = 0;
        char* pool = static_cast<char*>(g->stage_take(b->raw_bases + 64, &stage_bytes));
        struct StageGuard { rtk_graph* g; void* p; uint64_t n; ~StageGuard() { g->stage_give(p, n); } } guard = {g, pool, stage_bytes};
        auto pack_range = [&](uint32_t lo, uint32_t hi) { for (uint32_t i = lo; i < hi; ++i) if (raw_len[i]) memcpy(pool + ro[i], raw[i], raw_len[i]); };
        {
            const uint32_t n_thr = (b->raw_bases >= (4u << 20) && n >= 8) ? 4u : 1u;
            std::vector<uint32_t> cut(n_thr + 1, n); cut[0] = 0;
            for (uint32_t t = 1, i = 0; t < n_thr; ++t) { const uint64_t want = b->raw_bases / n_thr * t; while (i < n && ro[i] < want) ++i; cut[t] = i; }
            std::vector<std::thread> thr;
            for (uint32_t t = 1; t < n_thr; ++t) thr.emplace_back(pack_range, cut[t], cut[t + 1]);
            pack_range(cut[0], cut[1]);
            for (size_t t = 0; t < thr.size(); ++t) thr[t].join();
        }
        memset(pool + b->raw_bases, 'N', 64);
        b->d_raw = b->alloc<char>(b->raw_bases + 64); b->d_raw_off = b->alloc<uint64_t>(n + 1);
        rtk_h2d_s(b->d_raw, pool, b->raw_bases + 64, b->stream); rtk_h2d_s(b->d_raw_off, ro.data(), 8ull * (n + 1), b->stream);
        rtk_ssync(b->stream); // the staging buffer goes back to the pool
        b->has_raw = true;
    } catch (const std::exception& e) { rtk_batch_free(b); *out = nullptr; return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return RTK_OK;
}

RTK_GLOBAL void k_phase(const LaunchCtx* L, GraphView g, OptsView o, BatchView bv, PhaseView pv, char* scratch, uint64_t stride, RegionScratchCfg cfg, int grid, int only_flagged, const uint32_t* list, uint32_t n_list) {
#ifdef RTK_SIM
    RegionScratch hdr;
#else
    __shared__ RegionScratch hdr;
#endif
    RegionScratch* sc = region_scratch_carve(scratch + static_cast<uint64_t>(RTK_BLOCK_ID) * stride, cfg, &hdr);
    rtk_sync();
    (void)o;
    RCtx c = {L->g, L->o, L->bv, L->rb, {rtk_opaque(sc)}, {g.k}};
    for (uint32_t ri = static_cast<uint32_t>(RTK_BLOCK_ID); ri < n_list; ri += static_cast<uint32_t>(grid)) { // list: the reads of this kernel, longest first
        const uint32_t r = list[ri];
        if (only_flagged && bv.status[r] == 0) continue;
        *sc->overflow = 0; sc->top[RTK_ARENA_REGION] = 0;
        rtk_phase_read(c, pv, r);
        if (rtk_lane() == 0) bv.status[r] = *sc->overflow;
    }
}

// fixSNPs() of every read of a second-pass batch, in place (`-f`, src/Ratatosk.cpp:828); work: RTK_FIXSNPS_WIN bytes per wave
RTK_GLOBAL void k_fix_snps(GraphView g, BatchView bv, unsigned char* work, int grid) {
    unsigned char* win = work + static_cast<uint64_t>(RTK_BLOCK_ID) * RTK_FIXSNPS_WIN;
    for (uint32_t ri = static_cast<uint32_t>(RTK_BLOCK_ID); ri < bv.n_reads; ri += static_cast<uint32_t>(grid)) {
        const uint32_t r = bv.order[ri];
        // (the reads are rewritten in place: the pointer is taken as a plain global one, not through U<const char*>::get(), whose constant address space would let the
        // compiler keep earlier loads of the read across these stores; no U<const T*> field may alias memory the same launch writes)
        rtk_fix_snps_read(g, rtk_gp(const_cast<char*>(rtk_u(bv.seq.v))) + bv.roff[r], static_cast<uint32_t>(bv.roff[r + 1] - bv.roff[r]), win);
    }
}

// reads re-packed in read order after the pre-filter: new sequence + quality pools
RTK_GLOBAL void k_repack(BatchView bv, PhaseView pv, char* seq, char* qual, const uint64_t* new_off, int grid) {
    for (uint32_t r = static_cast<uint32_t>(RTK_BLOCK_ID); r < bv.n_reads; r += static_cast<uint32_t>(grid)) {
        const uint64_t src = pv.out_off[r]; const uint32_t l = pv.out_len[r]; const uint64_t dst = new_off[r];
        for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < l; i += RTK_WAVE) { seq[dst + i] = pv.out_pool[src + i]; qual[dst + i] = pv.out_pool[src + l + i]; }
    }
}

static RegionScratchCfg region_cfg(uint32_t max_len_exact, int attempt);

// work area of one wave (or workgroup) of the phasing step for reads of at most max_len characters (raw or corrected): the buffers the
// read program touches (two output strings, three position bitmaps, the Bloom filters in arena 0, the run lists) and the alignment
// scratch for a whole-read problem; everything else of the region stage's layout at its minimum. attempt > 0: 8x / 64x of it.
static RegionScratchCfg phase_cfg(uint32_t max_len_exact, int attempt) {
    uint32_t max_len = 8192u; while (max_len < max_len_exact) max_len <<= 1;
    const uint32_t scale = 1u << (3 * attempt);
    RegionScratchCfg c;
    c.str_cap = (2u * max_len + 4096u) * scale;
    c.my.w_cap = c.str_cap / 64 + 2; c.my.t_cap = c.str_cap; c.my.r_cap = c.str_cap; c.my.mv_cap = 2 * c.str_cap;
    c.my.tb_cap_words = std::max<uint64_t>(4ull * 52429 + 64, 4ull * c.my.w_cap + 64); // 1 MB tables of the leaf tracebacks, or the final vectors of a pass
    c.set_cap = 4096u * scale; c.um_cap = 64u * scale; c.list_cap = std::max<uint32_t>(1024u, max_len / 8u) * scale; c.memo_cap = 64u * scale;
    c.bm_words = (2u * max_len) / 64 + 16; c.arena_cap = std::max<uint64_t>(256ull << 10, 32ull * max_len) * scale;
    return c;
}

static void fix_snps_step(rtk_batch* b) {
    const int grid = std::min<int>(default_grid(), b->n > 0 ? static_cast<int>(b->n) : 1);
    unsigned char* work = b->alloc<unsigned char>(static_cast<uint64_t>(grid) * RTK_FIXSNPS_WIN);
    rtk_launch(k_fix_snps, grid, b->stream, b->g->dview, b->bv, work, grid);
    b->snps_fixed = true;
}

// stage entry: fixSNPs() of one read (upper-cased first, as the worker does before it: src/Ratatosk.cpp:814); out: len characters
extern "C" int rtk_fix_snps(rtk_graph* g, const char* seq, uint32_t len, char* out) {
    if (!g || !seq || !out) return rtk_fail(RTK_ERR_ARG, "rtk_fix_snps: null argument");
    if (!g->on_device) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_fix_snps: graph is not resident on a device (call rtk_graph_upload)");
    try {
        rtk_set_device(g->device);
        std::string up(seq, len);
        for (size_t i = 0; i < up.size(); ++i) up[i] = static_cast<char>(toupper(static_cast<unsigned char>(up[i])));
        char* dseq = static_cast<char*>(rtk_dmalloc(len + 64));
        uint64_t* droff = static_cast<uint64_t*>(rtk_dmalloc(16));
        uint32_t* dord = static_cast<uint32_t*>(rtk_dmalloc(4));
        unsigned char* work = static_cast<unsigned char*>(rtk_dmalloc(RTK_FIXSNPS_WIN));
        const uint64_t roff[2] = {0, len}; const uint32_t ord = 0;
        if (len) rtk_h2d(dseq, up.data(), len);
        rtk_h2d(droff, roff, 16); rtk_h2d(dord, &ord, 4);
        BatchView bv; memset(&bv, 0, sizeof(bv));
        bv.n_reads = 1; bv.n_bases = len; bv.seq = dseq; bv.roff = droff; bv.order = dord;
        rtk_launch(k_fix_snps, 1, 0, g->dview, bv, work, 1);
        rtk_dsync();
        if (len) rtk_d2h(out, dseq, len);
        rtk_dfree(dseq); rtk_dfree(droff); rtk_dfree(dord); rtk_dfree(work);
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return RTK_OK;
}

// phasing() of every read (src/Ratatosk.cpp:832), then the batch is rebuilt around the reads it returns
static int phase_step(rtk_batch* b, const OptsView& ov) {
    rtk_graph* g = b->g;
    BatchView& bv = b->bv;
    const rtk_stream_t st = b->stream;
    const int grid = default_grid();
    rtk_dzero_s(bv.hitmap, 8ull * (b->n_bases / 64 + 4), st); rtk_dzero_s(bv.status, 4ull * b->n, st); rtk_dzero_s(bv.counters, 8 * RTK_CNT_TOTAL, st);
    { const int xgrid = 2 * grid; rtk_launch(k_lookup_exact, xgrid, st, g->dview, bv.seq, bv.roff, bv.n_reads, bv.n_bases, xgrid, bv.hits.get(), bv.hitmap.get(), reinterpret_cast<uint64_t*>(bv.counters + RTK_CNT_PROBES_EXACT)); }
    uint32_t max_len = b->raw_max_len; for (uint32_t i = 0; i < b->n; ++i) max_len = std::max<uint32_t>(max_len, static_cast<uint32_t>(b->roff[i + 1] - b->roff[i]));
    PhaseView pv;
    pv.raw = b->d_raw; pv.raw_off = b->d_raw_off;
    pv.out_cap = 2ull * (b->n_bases + b->raw_bases) + 4096; pv.out_pool = b->alloc<char>(pv.out_cap); pv.out_top = b->alloc<unsigned long long>(1);
    pv.out_off = b->alloc<uint64_t>(b->n); pv.out_len = b->alloc<uint32_t>(b->n);
    { // TinyBloomFilter(nb_elem, 14): number of hash functions (src/TinyBloomFilter.hpp:17-19), in double like the reference
        const double bpe = 14.0; uint64_t nb_h = static_cast<uint64_t>(bpe * std::log(2.0));
        auto fpp = [&](uint64_t h) { const double h_d = static_cast<double>(h); return std::pow(1.0 - std::exp(-(h_d / bpe)), h_d); };
        nb_h += static_cast<uint64_t>(fpp(nb_h) >= fpp(nb_h + 1));
        pv.tbf_nb_h = static_cast<uint32_t>(nb_h & 0xffull); }
    pv.align_all = rtk_knob_phase_align_all() ? 1u : 0u;
    rtk_dzero_s(pv.out_top, 8, st);
    struct Slab { rtk_graph* g; void* p; uint64_t n; ~Slab() { if (p) g->phase_give(p, n); } } slab = {g, nullptr, 0}; // this ticket's own work area (no graph-wide lock)
    // Three classes of reads, longest first inside each. The whole-read alignment of phasing() is linear in the read length per Hirschberg level
    // since it is banded, and the passes of a level share the lanes of a wave (rtk_myers_lvl.h): one wave per read is the efficient schedule.
    // What a second wave buys is latency, and only the longest reads of a ticket decide how long its launch lasts:
    //   short  (<= 8 kb)               one wave per read, small work areas
    //   mid    (<= RTK_PHASE_LONG)     one wave per read, work areas for the longest of them
    //   long   (>  RTK_PHASE_LONG)     4 waves per read (k_phase_long; RTK_PHASE_LWAVES): gangs / row blocks of a level and the leaf tracebacks side by side
    std::vector<uint32_t> l_short, l_long, l_mid;
    {
        const uint32_t thr = rtk_knob_phase_long(); // 0: no multi-wave class
        const uint32_t thr_s = 8192; (void)thr_s;
        std::vector<uint64_t> roff_raw(b->n + 1); rtk_d2h_s(roff_raw.data(), b->d_raw_off, 8ull * (b->n + 1), st);
        std::vector<uint32_t> ord(b->n); rtk_d2h_s(ord.data(), bv.order, 4ull * b->n, st);
        for (uint32_t i = 0; i < b->n; ++i) {
            const uint32_t r = ord[i]; const uint64_t lc = b->roff[r + 1] - b->roff[r], lr = roff_raw[r + 1] - roff_raw[r]; const uint64_t lm = std::max(lc, lr);
#ifdef RTK_SIM
            (void)thr; (void)lm; l_short.push_back(r);
#else
            (lm <= thr_s ? l_short : ((thr && lm > thr) ? l_long : l_mid)).push_back(r);
#endif
        }
    }
    uint32_t* d_list = b->alloc<uint32_t>(b->n + 1);
    if (!l_short.empty()) rtk_h2d(d_list, l_short.data(), 4ull * l_short.size());
    if (!l_long.empty()) rtk_h2d(d_list + l_short.size(), l_long.data(), 4ull * l_long.size());
    if (!l_mid.empty()) rtk_h2d(d_list + l_short.size() + l_long.size(), l_mid.data(), 4ull * l_mid.size());
    // longest read (raw or corrected) of each class: its work areas are sized for it
    uint32_t cmax[3] = {0, 0, 0};
    { std::vector<uint64_t> roff_raw(b->n + 1); rtk_d2h_s(roff_raw.data(), b->d_raw_off, 8ull * (b->n + 1), st);
      const std::vector<uint32_t>* cl[3] = {&l_short, &l_long, &l_mid};
      for (int ci = 0; ci < 3; ++ci) for (size_t x = 0; x < cl[ci]->size(); ++x) { const uint32_t r = (*cl[ci])[x]; cmax[ci] = std::max<uint32_t>(cmax[ci], static_cast<uint32_t>(std::max<uint64_t>(b->roff[r + 1] - b->roff[r], roff_raw[r + 1] - roff_raw[r]))); } }
    { RegionBatch none; memset(&none, 0, sizeof(none)); rtk_launch(k_set_ctx, 1, st, b->ctx(), g->dview, ov, bv, none); } // the views the read programs see (no region list yet)
    for (int attempt = 0; attempt < 3; ++attempt) {
        const RegionScratchCfg cfg_s = phase_cfg(cmax[0], attempt), cfg_l = phase_cfg(cmax[1], attempt), cfg_m = phase_cfg(cmax[2], attempt);
#ifdef RTK_SIM
        const uint64_t stride_s = region_scratch_bytes(cfg_s), stride_l = region_scratch_bytes(cfg_l), stride_m = region_scratch_bytes(cfg_m);
        int pgrid = 16; const int lwaves = 1;
#else
        // waves per workgroup of the long class. A second-pass run is bound by wave slots (128 VGPRs: 4096 waves on the chip, several tickets in flight) and
        // the helpers of a workgroup idle most of the time since the passes are banded: 4 waves x 192 workgroups instead of 16 x 64 is +15-20 % on the
        // file-to-file rate (profiles/scripts/p2_sweep.sh); the longest read of a ticket takes longer, other tickets fill the time
        const int lwaves = rtk_knob_phase_lwaves();
        const uint64_t stride_s = region_scratch_bytes(cfg_s), stride_l = rtk_phase_long_stride(cfg_l, lwaves), stride_m = region_scratch_bytes(cfg_m);
        int pgrid = attempt == 0 ? rtk_knob_phase_pgrid() : (attempt == 1 ? 128 : 8);
#endif
        pgrid = static_cast<int>(std::min<uint32_t>(static_cast<uint32_t>(pgrid), l_short.empty() ? 1u : static_cast<uint32_t>(l_short.size())));
        int lgrid = attempt == 0 ? rtk_knob_phase_lgrid() : (attempt == 1 ? 16 : 4); // workgroups of `lwaves` waves
        lgrid = static_cast<int>(std::min<uint32_t>(static_cast<uint32_t>(lgrid), l_long.empty() ? 1u : static_cast<uint32_t>(l_long.size())));
        int mgrid = attempt == 0 ? rtk_knob_phase_mgrid() : (attempt == 1 ? 64 : 4);
        mgrid = static_cast<int>(std::min<uint32_t>(static_cast<uint32_t>(mgrid), l_mid.empty() ? 1u : static_cast<uint32_t>(l_mid.size())));
        const uint64_t off_l = stride_s * static_cast<uint64_t>(pgrid), off_m = off_l + (l_long.empty() ? 0u : stride_l * static_cast<uint64_t>(lgrid));
        const uint64_t need = off_m + (l_mid.empty() ? 0u : stride_m * static_cast<uint64_t>(mgrid));
        if (slab.n < need) { if (slab.p) { g->phase_give(slab.p, slab.n); slab.p = nullptr; slab.n = 0; } slab.p = g->phase_take(need, &slab.n); }
        char* scratch = static_cast<char*>(slab.p);
        const auto tp0 = std::chrono::steady_clock::now();
#ifndef RTK_SIM
        rtk_stream_t aux = nullptr, aux2 = nullptr; // the kernels side by side: the long reads first (they decide how long the step lasts)
        if (!l_long.empty() || !l_mid.empty()) rtk_ssync(st);
        if (!l_long.empty()) { aux = rtk_stream_create(); rtk_launch_phase_long(lgrid, lwaves, aux, b->ctx(), g->dview, ov, bv, pv, scratch + off_l, stride_l, cfg_l, d_list + l_short.size(), static_cast<uint32_t>(l_long.size()), attempt == 0 ? 0 : 1); }
        if (!l_mid.empty()) { aux2 = rtk_stream_create(); rtk_launch(k_phase, mgrid, aux2, static_cast<const LaunchCtx*>(b->ctx()), g->dview, ov, bv, pv, scratch + off_m, stride_m, cfg_m, mgrid, attempt == 0 ? 0 : 1, static_cast<const uint32_t*>(d_list + l_short.size() + l_long.size()), static_cast<uint32_t>(l_mid.size())); }
#endif
        if (!l_short.empty()) rtk_launch(k_phase, pgrid, st, static_cast<const LaunchCtx*>(b->ctx()), g->dview, ov, bv, pv, scratch, stride_s, cfg_s, pgrid, attempt == 0 ? 0 : 1, static_cast<const uint32_t*>(d_list), static_cast<uint32_t>(l_short.size()));
#ifndef RTK_SIM
        { std::string err;
          if (aux) { try { rtk_ssync(aux); } catch (const std::exception& e) { err = e.what(); } rtk_stream_destroy(aux); }
          if (aux2) { try { rtk_ssync(aux2); } catch (const std::exception& e) { err = e.what(); } rtk_stream_destroy(aux2); }
          if (!err.empty()) throw std::runtime_error(err); }
#endif
        rtk_ssync(st);
        if (rtk_knob_trace()) fprintf(stderr, "[rtk trace] phase attempt %d: %.2f ms (k_phase %d waves for %zu reads <= 8 kb and %d waves for %zu longer ones, k_phase_long %d x %d for %zu reads, work areas %.1f GB), %llu + %llu bases\n", attempt, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count(), pgrid, l_short.size(), l_mid.empty() ? 0 : mgrid, l_mid.size(), lwaves, l_long.empty() ? 0 : lgrid, l_long.size(), need / 1073741824.0, static_cast<unsigned long long>(b->n_bases), static_cast<unsigned long long>(b->raw_bases));
        { unsigned long long sk = 0; rtk_d2h_s(&sk, bv.counters + RTK_CNT_PHASE_SKIPPED, sizeof(sk), st); b->stats.n_phase_skipped = sk; b->stats.ms_phase = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count();
          if (rtk_knob_trace()) fprintf(stderr, "[rtk trace] phase: whole-read alignment skipped for %llu of %u reads (no unsupported stretch)\n", sk, b->n); }
        if (rtk_knob_trace()) { unsigned long long pc[RTK_CNT_PHASE_TRACE_END - RTK_CNT_PHASE_TRACE]; rtk_d2h_s(pc, bv.counters + RTK_CNT_PHASE_TRACE, sizeof(pc), st);
            fprintf(stderr, "[rtk trace] k_phase_long wave-0 cycles: alignments %.3g, of which Hirschberg driver %.3g (half passes %.3g, columns + split %.3g, leaf tracebacks %.3g)\n", double(pc[0]), double(pc[4]), double(pc[1]), double(pc[2]), double(pc[3])); }
        std::vector<uint32_t> stt(b->n); rtk_d2h_s(stt.data(), bv.status, 4ull * b->n, st);
        bool ovf = false; for (uint32_t i = 0; i < b->n; ++i) if (stt[i]) ovf = true;
        if (ovf && rtk_knob_trace()) { std::map<uint32_t, std::pair<uint32_t, uint32_t> > hist; for (uint32_t i = 0; i < b->n; ++i) if (stt[i]) { auto& h = hist[stt[i]]; ++h.first; h.second = std::max<uint32_t>(h.second, static_cast<uint32_t>(b->roff[i + 1] - b->roff[i])); }
            fprintf(stderr, "[rtk trace] phase attempt %d: reads to do again by status code:", attempt); for (auto& kv : hist) fprintf(stderr, " [code %u: %u reads, longest %u]", kv.first, kv.second.first, kv.second.second); fprintf(stderr, "\n"); }
        if (!ovf) break;
        if (attempt == 2) return rtk_fail(RTK_ERR_DEVICE, "phasing: scratch capacity exceeded after 3 attempts");
    }
    unsigned long long out_top = 0; rtk_d2h_s(&out_top, pv.out_top, 8, st);
    if (out_top > pv.out_cap) return rtk_fail(RTK_ERR_DEVICE, "phasing: output pool exhausted");
    std::vector<uint32_t> ol(b->n); rtk_d2h_s(ol.data(), pv.out_len, 4ull * b->n, st);
    // the batch again, around the new reads
    for (uint32_t i = 0; i < b->n; ++i) b->roff[i + 1] = b->roff[i] + ol[i];
    const uint64_t new_bases = b->roff[b->n];
    char* nseq = b->alloc<char>(new_bases + 64); char* nqual = b->alloc<char>(new_bases + 64);
    uint64_t* nroff = b->alloc<uint64_t>(b->n + 1); uint32_t* nord = b->alloc<uint32_t>(b->n);
    { std::vector<uint32_t> ord(b->n); for (uint32_t i = 0; i < b->n; ++i) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return ol[x] > ol[y]; });
      rtk_h2d(nroff, b->roff.data(), 8ull * (b->n + 1)); rtk_h2d(nord, ord.data(), 4ull * b->n); }
    { std::vector<char> pad(64, 'N'); rtk_h2d(nseq + new_bases, pad.data(), 64); std::vector<char> padq(64, '!'); rtk_h2d(nqual + new_bases, padq.data(), 64); }
    { const int rg = std::min<int>(grid, static_cast<int>(b->n) > 0 ? static_cast<int>(b->n) : 1); rtk_launch(k_repack, rg, st, bv, pv, nseq, nqual, nroff, rg); }
    rtk_ssync(st);
    bv.seq = nseq; bv.qual = nqual; bv.roff = nroff; bv.order = nord; bv.n_bases = new_bases; b->n_bases = new_bases;
    b->alloc_arrays();
    b->rb.seq_rc = nullptr; // region-stage buffers are sized by the batch: allocated again
    b->phased = true;
    return RTK_OK;
}

#include "rtk_pipeline_run.inc"
