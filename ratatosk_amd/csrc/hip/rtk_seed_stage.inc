// Anchor ("seed") stage of a batch (stage A of the pipeline): its kernels over the programs of rtk_seeds.h, and the host steps that launch them.
// (included by rtk_pipeline.inc; k_lookup_exact, the first kernel of the stage, stands in rtk_device.hip: the stage entries use it as well)

// ------------------------------------------------------------------------------------------------ kernels
// The per-read seed programs read the views through the launch's LaunchCtx and their work-area descriptor from LDS: a by-value copy on
// the wave's stack is 64 interleaved copies that every field read fetches a 256-byte row of.
#ifdef RTK_SIM
#define RTK_SEED_SCRATCH(sc, expr) const SeedScratch sc = (expr)
#else
#define RTK_SEED_SCRATCH(sc, expr) __shared__ SeedScratch sc; sc = (expr); __syncthreads()
#endif
// One work item = one segment of `seg_w` windows of a read (`items`: read << 32 | segment, the segments of the longest reads first; built by rtk_batch_create).
RTK_GLOBAL void k_mask(const LaunchCtx* L, BatchView bv, const uint64_t* items, uint32_t n_items, uint32_t seg_w, char* scratch, uint64_t stride, SeedScratchCfg cfg, int grid) {
    RTK_SEED_SCRATCH(sc, seed_scratch_carve(scratch + static_cast<uint64_t>(RTK_BLOCK_ID) * stride, cfg));
    for (uint32_t it = static_cast<uint32_t>(RTK_BLOCK_ID); it < n_items; it += static_cast<uint32_t>(grid)) {
        const uint64_t e = rtk_u(items[it]);
        const uint32_t r = static_cast<uint32_t>(e >> 32), seg = static_cast<uint32_t>(e & 0xFFFFFFFFull);
        *sc.overflow = 0;
        rtk_mask_read(L->g, L->o, L->bv, sc, r, seg * seg_w, (seg + 1u) * seg_w);
        if (*sc.overflow && rtk_lane() == 0) rtk_atomic_or(bv.status.get() + r, 1u);
    }
}

// 1-edit search. Two kernels so that the register budget of the variant-spelling fallback does not cap the occupancy of the seeded search.
template <int ENUMERATE>
RTK_DEV void inexact_body(const LaunchCtx* L, const BatchView& bv, int grid) {
    const GraphView& g = L->g;
    const uint64_t n_tiles = (bv.n_bases + 63) / 64;
    unsigned long long probes = 0, slots = 0, hits = 0;
    PoolChunk chunk; chunk.base = 0; chunk.left = 0;
    for (uint64_t t = static_cast<uint64_t>(RTK_BLOCK_ID); t < n_tiles; t += static_cast<uint64_t>(grid)) {
        if (ENUMERATE) rtk_inexact_tile(g, L->bv, t, &probes, &slots, &hits, &chunk, L->o.a2_exclusive);
        else rtk_inexact_tile_seeded(g, L->bv, t, &probes, &slots, &hits, &chunk, L->o.a2_exclusive, L->o.inexact_route);
    }
    // wave reduction of the per-lane probe tallies, then one atomic per wave
    unsigned long long tot = probes, tots = slots;
#ifndef RTK_SIM
    for (int o = 32; o > 0; o >>= 1) { tot += __shfl_xor(tot, o, 64); tots += __shfl_xor(tots, o, 64); }
#endif
    if (rtk_lane() == 0) { if (tot) rtk_atomic_add(bv.counters + RTK_CNT_PROBES_INEXACT, tot); if (tots) rtk_atomic_add(bv.counters + RTK_CNT_SLOTS_INEXACT, tots); if (hits) rtk_atomic_add(bv.counters + RTK_CNT_HITS_INEXACT, hits); }
}
// half-k-mer seeds + verification (default)
#ifndef RTK_SIM
#ifndef RTK_INEXACT_WPE
#define RTK_INEXACT_WPE 6
#endif
__attribute__((amdgpu_waves_per_eu(RTK_INEXACT_WPE, RTK_INEXACT_WPE)))
#endif
RTK_GLOBAL void k_inexact(const LaunchCtx* L, BatchView bv, int grid) { inexact_body<0>(L, bv, grid); }
// every 1-edit variant spelled and probed (RTK_INEXACT_ENUM=1 cross-check; fallback when the half-k-mer index is not built)
RTK_GLOBAL void k_inexact_enum(const LaunchCtx* L, BatchView bv, int grid) { inexact_body<1>(L, bv, grid); }

RTK_GLOBAL void k_finalize(const LaunchCtx* L, BatchView bv, char* scratch, uint64_t stride, SeedScratchCfg cfg, int grid) {
    RTK_SEED_SCRATCH(sc, seed_scratch_carve(scratch + static_cast<uint64_t>(RTK_BLOCK_ID) * stride, cfg));
    for (uint32_t ri = static_cast<uint32_t>(RTK_BLOCK_ID); ri < bv.n_reads; ri += static_cast<uint32_t>(grid)) {
        const uint32_t r = bv.order[ri];
        *sc.overflow = 0;
        rtk_finalize_read(L->g, L->o, L->bv, sc, r);
        if (*sc.overflow && rtk_lane() == 0) bv.status[r] |= 2u;
    }
}

// ------------------------------------------------------------------------------------------------ host side
// seed_stage_checked (below) calls these steps in order, once per attempt; what they hand on to each other lives in SeedRun.
struct SeedRun {
    rtk_batch* b; OptsView ov; rtk_stream_t st;
    int attempt;    // 0, then 1 and 2 with work areas 4x / 16x as large on few waves
    bool second_pass; // getSeeds keeps the exact hits only (src/Graph.cpp:100): no masked copy, no 1-edit search
    int grid;       // the kernels that walk tiles of 64 positions
    int rgrid, mgrid; // k_finalize: one wave per read at a time; k_mask: one wave per segment of a read
    SeedScratchCfg cfg; uint64_t stride; char* scratch; // the work area of one wave of k_mask / k_finalize, and those of all waves
    RtkTimer t_exact, t_mask, t_inexact, t_finalize;
    const LaunchCtx* ctx() const { return static_cast<const LaunchCtx*>(b->ctx()); }
};

static int seed_waves() { return rtk_knob_seed_waves(); } // waves of the per-read seed kernels (one read each at a time, longest first): 16 per CU fit (LDS); 1024 -> 4096: k_mask 1.5 -> 1.0 ms, k_finalize 4.7 -> 3.0 ms per 64 Mb, 13 GB of work areas

// what the stage writes without having read it: presence bits, raw-hit descriptors, the tops of the two pools, the reads' status words, the counters
static void seed_clear(SeedRun& R) {
    rtk_batch* b = R.b; BatchView& bv = b->bv; const rtk_stream_t st = R.st;
    rtk_dzero_s(bv.hitmap, 8ull * (b->n_bases / 64 + 4), st); rtk_dzero_s(bv.wdesc, 8ull * (b->n_bases + 64), st); rtk_dzero_s(bv.ipool_top, 8, st); rtk_dzero_s(bv.wk_top, 8, st); rtk_dzero_s(bv.status, 4ull * b->n, st); rtk_dzero_s(bv.counters, 8 * RTK_CNT_TOTAL, st);
}

static void seed_exact(SeedRun& R) {
    BatchView& bv = R.b->bv;
    R.t_exact.start(R.st);
    const int xgrid = 2 * R.grid; // 26 VGPRs: eight waves per SIMD fit
    rtk_launch(k_lookup_exact, xgrid, R.st, R.b->g->dview, bv.seq, bv.roff, bv.n_reads, bv.n_bases, xgrid, bv.hits.get(), bv.hitmap.get(), reinterpret_cast<uint64_t*>(bv.counters + RTK_CNT_PROBES_EXACT)); // queries there, table slots at RTK_CNT_SLOTS_EXACT
    R.t_exact.stop(R.st);
}

// waves of a per-read kernel over n_items work items: every attempt after the first runs on 64 (its work areas are 4x / 16x as large)
static int seed_wave_grid(uint32_t n_items, int attempt) {
    int grid = static_cast<int>(std::min<uint32_t>(n_items, static_cast<uint32_t>(attempt ? 64 : seed_waves())));
#ifdef RTK_SIM
    grid = std::min(grid, 16);
#endif
    return grid < 1 ? 1 : grid;
}

// the work areas of k_mask and k_finalize, their two grids, and the views of the launches that follow
static void seed_size(SeedRun& R) {
    rtk_batch* b = R.b; const int attempt = R.attempt;
    SeedScratchCfg& cfg = R.cfg;
    cfg.set_cap = 32768u << (2 * attempt); cfg.v_cap = 32768u << (2 * attempt);
    if (attempt == 0 && rtk_knob_test_tiny_scratch()) { cfg.set_cap = 48; cfg.v_cap = 64; } // test hook, see region_cfg
    uint32_t max_len = 0; for (uint32_t i = 0; i < b->n; ++i) max_len = std::max<uint32_t>(max_len, static_cast<uint32_t>(b->roff[i + 1] - b->roff[i]));
    { uint32_t q = 131072u; while (q < max_len) q <<= 1; cfg.s_cap = q + 64; } // coarse steps, see region_cfg
    R.stride = seed_scratch_bytes(cfg);
    R.rgrid = seed_wave_grid(b->n, attempt);
    R.mgrid = seed_wave_grid(b->n_mask_items, attempt);
    R.scratch = graph_scratch(b->g, 0, R.stride * std::max(R.rgrid, R.mgrid));
    { RegionBatch none; memset(&none, 0, sizeof(none)); rtk_launch(k_set_ctx, 1, R.st, b->ctx(), b->g->dview, R.ov, b->bv, none); }
}

static void seed_mask(SeedRun& R) {
    rtk_batch* b = R.b; BatchView& bv = b->bv;
    R.t_mask.start(R.st);
    if (!R.second_pass) { // the masked copy starts as all 'N'; the segments of the reads (long reads: several waves each) open the gaps
        rtk_dfill_s(bv.masked, 'N', b->n_bases + 64, R.st);
        if (b->n_mask_items) rtk_launch(k_mask, R.mgrid, R.st, R.ctx(), bv, static_cast<const uint64_t*>(b->d_mask_items), b->n_mask_items, b->mask_seg, R.scratch, R.stride, R.cfg, R.mgrid);
    }
    R.t_mask.stop(R.st);
}

static void seed_inexact(SeedRun& R) {
    BatchView& bv = R.b->bv; const int grid = R.grid;
    R.t_inexact.start(R.st);
    if (!R.second_pass) { if (rtk_knob_inexact_enum() || R.b->g->dview.hx_mask == 0) rtk_launch(k_inexact_enum, grid, R.st, R.ctx(), bv, grid); else { const int sgrid = grid + grid / 2; rtk_launch(k_inexact, sgrid, R.st, R.ctx(), bv, sgrid); } } // 76 VGPRs: six waves per SIMD (eight measured the same)
    R.t_inexact.stop(R.st);
}

static void seed_finalize(SeedRun& R) {
    R.t_finalize.start(R.st);
    rtk_launch(k_finalize, R.rgrid, R.st, R.ctx(), R.b->bv, R.scratch, R.stride, R.cfg, R.rgrid);
    R.t_finalize.stop(R.st);
}

// waits for the stage and reads its four kernel times
static void seed_times(SeedRun& R) {
    rtk_ssync(R.st);
    rtk_stats& s = R.b->stats;
    s.ms_lookup_exact = R.t_exact.elapsed(); s.ms_mask = R.t_mask.elapsed(); s.ms_lookup_inexact = R.t_inexact.elapsed(); s.ms_seeds = R.t_finalize.elapsed();
}

// the phases of rtk_finalize_read (rtk_seed_finalize.h) in the order of its RTK_PHASE() calls: slot i of RTK_CNT_FINALIZE and of RTK_CNT_FINALIZE_SLOWEST_PHASES
static const char* const seed_finalize_phases[7] = {"solid", "junction", "gather", "classify+sort", "groups", "conflicts", "write"};
static_assert(RTK_CNT_FINALIZE_SLOWEST - RTK_CNT_FINALIZE == 7 && RTK_CNT_FINALIZE_SLOWEST_PHASES_END - RTK_CNT_FINALIZE_SLOWEST_PHASES == 7, "one counter per phase of k_finalize");

// the [rtk trace] lines of one attempt (profiles/scripts read them)
static void seed_trace(SeedRun& R, std::chrono::steady_clock::time_point w0) {
    unsigned long long c[RTK_CNT_FINALIZE_SLOWEST_PHASES_END]; rtk_d2h_s(c, R.b->bv.counters, sizeof(c), R.st);
    auto phases = [](const unsigned long long* v) { std::string s; char one[64]; for (int i = 0; i < 7; ++i) { snprintf(one, sizeof(one), " %s %.3g", seed_finalize_phases[i], double(v[i])); s += one; } return s; };
    fprintf(stderr, "[rtk trace] finalize, slowest read:%s cycles\n", phases(c + RTK_CNT_FINALIZE_SLOWEST_PHASES).c_str());
    fprintf(stderr, "[rtk trace] finalize wave-cycles:%s | slowest read %.3g cycles\n", phases(c + RTK_CNT_FINALIZE).c_str(), double(c[RTK_CNT_FINALIZE_SLOWEST]));
    const rtk_stats& s = R.b->stats;
    fprintf(stderr, "[rtk trace] seeds attempt %d: %.2f ms (kernels %.2f)\n", R.attempt, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count(), s.ms_lookup_exact + s.ms_mask + s.ms_lookup_inexact + s.ms_seeds);
}

// did a work area or a pool run out? *pools: one of the two pools did (RTK_CNT_OVERFLOW), not only a read's work area (its status word)
static bool seed_overflowed(SeedRun& R, bool* pools) {
    rtk_batch* b = R.b;
    std::vector<uint32_t> st(b->n);
    rtk_d2h_s(st.data(), b->bv.status, 4ull * b->n, R.st);
    unsigned long long cnt[RTK_CNT_SEED_READBACK]; rtk_d2h_s(cnt, b->bv.counters, sizeof(cnt), R.st);
    *pools = cnt[RTK_CNT_OVERFLOW] != 0;
    bool ovf = *pools;
    for (uint32_t i = 0; i < b->n; ++i) if (st[i]) ovf = true;
    return ovf;
}

// the raw-hit pool and the weak-anchor pool, four times as large (the old ones stay with the batch until it is freed)
static void seed_grow_pools(rtk_batch* b) {
    b->bv.ipool_cap *= 4; b->bv.ipool = b->alloc<uint64_t>(2 * b->bv.ipool_cap);
    b->bv.wk_cap *= 4; b->bv.wk_pos = b->alloc<uint32_t>(b->bv.wk_cap); b->bv.wk_hit = b->alloc<uint64_t>(b->bv.wk_cap);
}

// anchors of every read: exact scan, mask, inexact scan, filters. A capacity exceeded somewhere: grow and redo the stage (still on the device)
static int seed_stage_checked(rtk_batch* b, const OptsView& ov) {
    std::lock_guard<std::mutex> hold(b->g->scratch_lock[0]);
    SeedRun R; R.b = b; R.ov = ov; R.st = b->stream; R.second_pass = ov.long_read_correct != 0; R.grid = default_grid();
    for (R.attempt = 0; R.attempt < 3; ++R.attempt) {
        const auto w0 = std::chrono::steady_clock::now();
        seed_clear(R);
        seed_exact(R);
        seed_size(R);
        seed_mask(R);
        seed_inexact(R);
        seed_finalize(R);
        seed_times(R);
        if (rtk_knob_trace()) seed_trace(R, w0);
        bool pools = false;
        if (!seed_overflowed(R, &pools)) return RTK_OK;
        if (pools) seed_grow_pools(b);
    }
    return rtk_fail(RTK_ERR_DEVICE, "seed stage: scratch capacity exceeded after 3 attempts");
}
