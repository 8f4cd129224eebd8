// Batch run: seed stage -> region enumeration -> region correction (persistent waves) -> stitch; fetch; stats.
// (included by rtk_pipeline.inc)

RTK_GLOBAL void k_enum(const LaunchCtx* L, BatchView bv, int grid) {
#ifdef RTK_SIM
    unsigned char comp_tab[256];
#else
    __shared__ unsigned char comp_tab[256]; // the complement of every character (rtk_comp), looked up by the reverse complement of the reads
#endif
    for (uint32_t c = static_cast<uint32_t>(rtk_lane()); c < 256u; c += RTK_WAVE) comp_tab[c] = static_cast<unsigned char>(rtk_comp(static_cast<char>(c)));
    rtk_sync();
    for (uint32_t ri = static_cast<uint32_t>(RTK_BLOCK_ID); ri < bv.n_reads; ri += static_cast<uint32_t>(grid)) rtk_enum_regions(L->g, L->bv, L->rb, bv.order[ri], comp_tab); // longest reads first
}

// Dequeue order of the region kernel: long regions first (their cost grows super-linearly), so that the tail of the launch is made of cheap
// ones. One lane per region; heavy ones fill rorder[] from the front, light ones from the back (one atomic per class and wave).
// First pass only: the regions that need no graph walk at all -- reads returned whole, read ends on a solid anchor, gaps bridged by one unitig
// (src/Correction.cpp:814-858) or left as they are (:920-932): 74 % of the regions of configs[1] -- go to a list of their own (eorder) and are
// written by k_regions_easy, a kernel without work areas at full occupancy, instead of by the 128-register program of k_regions.
RTK_DEV bool rtk_region_is_heavy(const BatchView& bv, const RegionDesc& rd) {
    if (rd.kind == RTK_RG_GAP) { const uint32_t* sp = bv.s_pos + bv.roff[rd.read]; return (sp[rd.i_solid + 1] - sp[rd.i_solid]) >= 160u; }
    return rd.kind == RTK_RG_HEAD || rd.kind == RTK_RG_TAIL;
}
// the same-unitig shortcut of a gap (src/Correction.cpp:814-858): both anchors on one unitig and strand, in read order, the stretch between them
// within the length window. *shortcut = the unitig is copied; otherwise (and when the anchors overlap) the gap stays as it is. false: needs the search.
RTK_DEV bool rtk_gap_is_easy(const GraphView& g, const OptsView& o, const BatchView& bv, const RegionDesc& rd, bool* shortcut, UMap* ua_out, uint32_t* len_unitig_km_out, uint32_t* min_pos_out) {
    const uint64_t base = bv.roff[rd.read]; const uint32_t* sp = bv.s_pos + base; const uint32_t k = static_cast<uint32_t>(g.k);
    const uint32_t pa = sp[rd.i_solid], pb = sp[rd.i_solid + 1];
    const UMap ua = rtk_unpack_hit(bv.hits[base + pa]), ub = rtk_unpack_hit(bv.hits[base + pb]);
    *shortcut = false;
    bool same = (ua.unitig == ub.unitig) && (ua.strand == ub.strand);
    if (same && !(g.flags[ua.unitig] & RTK_F_SHORT_CYCLE)) {
        const uint32_t min_pos = ua.dist < ub.dist ? ua.dist : ub.dist, max_pos = ua.dist < ub.dist ? ub.dist : ua.dist;
        const uint32_t len_query_km = pb - pa, len_unitig_km = max_pos - min_pos;
        uint64_t mn, mx; rtk_min_max_len(len_unitig_km, o.weak_region_len_factor, &mn, &mx);
        same = same && ((ua.strand && (ua.dist < ub.dist)) || (!ua.strand && (ua.dist > ub.dist)));
        same = same && (len_query_km >= mn) && (len_query_km <= mx);
        *shortcut = same; *ua_out = ua; *len_unitig_km_out = len_unitig_km; *min_pos_out = min_pos;
        return true; // copied, or left uncorrected
    }
    return pb < pa + k; // overlapping anchors: left as it is; anything else is searched
}
#define RTK_OQ 4
RTK_GLOBAL void k_region_order(const LaunchCtx* L, uint64_t n_regions, int grid) {
    const BatchView& bv = L->bv; const RegionBatch& rb = L->rb;
    const bool first_pass = L->o.long_read_correct == 0;
    const uint32_t lane_max_gap = rb.lane_max_gap;
    // RTK_OQ chunks of 64 regions per step and ONE atomic per class and step: the three counters share a cache line, and 23 k atomics on it (one per
    // class and chunk of a 64 Mb step) were most of the kernel's 0.3 ms; the descriptor chains of the chunks of a step are in flight together
    for (uint64_t i0 = static_cast<uint64_t>(RTK_BLOCK_ID) * RTK_OQ * RTK_WAVE; i0 < n_regions; i0 += static_cast<uint64_t>(grid) * RTK_OQ * RTK_WAVE) {
        uint64_t mh[RTK_OQ], ml[RTK_OQ], me[RTK_OQ], mn[RTK_OQ][4]; uint32_t th = 0, tl = 0, te = 0, tn[4] = {0, 0, 0, 0}; // mn / tn: the lane kernel's class, by quarter of its gap range
#pragma unroll
        for (int q = 0; q < RTK_OQ; ++q) {
            const uint64_t i = i0 + static_cast<uint64_t>(q) * RTK_WAVE + static_cast<uint64_t>(rtk_lane());
            const bool in = i < n_regions;
            bool easy = false, heavy = false, lane_cls = false; uint32_t lane_sub = 0;
            if (in) {
                const RegionDesc rd = rb.regions[i];
                if (first_pass) {
                    if (rd.kind == RTK_RG_GAP) { bool sc_; UMap ua_; uint32_t a_, b_; easy = rtk_gap_is_easy(L->g, L->o, bv, rd, &sc_, &ua_, &a_, &b_); }
                    else easy = rd.kind == RTK_RG_WHOLE_MAX || rd.kind == RTK_RG_WHOLE_MIN || rd.kind == RTK_RG_TAIL_COPY;
                }
                if (first_pass && !easy && lane_max_gap != 0 && rd.kind == RTK_RG_GAP) { const uint32_t* sp = bv.s_pos + bv.roff[rd.read]; const uint32_t gl = sp[rd.i_solid + 1] - sp[rd.i_solid]; lane_cls = gl < lane_max_gap; lane_sub = lane_cls ? (4u * gl) / lane_max_gap : 0u; } // the lane-per-region kernel's class
                heavy = !easy && !lane_cls && rtk_region_is_heavy(bv, rd);
            }
            mh[q] = rtk_ballot(heavy); ml[q] = rtk_ballot(in && !heavy && !easy && !lane_cls); me[q] = rtk_ballot(easy);
            for (uint32_t sb = 0; sb < 4; ++sb) { mn[q][sb] = rtk_ballot(lane_cls && lane_sub == sb); tn[sb] += static_cast<uint32_t>(rtk_popc(mn[q][sb])); }
            th += static_cast<uint32_t>(rtk_popc(mh[q])); tl += static_cast<uint32_t>(rtk_popc(ml[q])); te += static_cast<uint32_t>(rtk_popc(me[q]));
        }
        unsigned long long bh = 0, bl = 0, be = 0, bn[4] = {0, 0, 0, 0};
        if (rtk_lane() == 0) {
            if (th) bh = rtk_atomic_add(rb.n_heavy.get(), static_cast<unsigned long long>(th));
            if (tl) bl = rtk_atomic_add(rb.n_heavy.get() + 1, static_cast<unsigned long long>(tl));
            if (te) be = rtk_atomic_add(rb.n_heavy.get() + 2, static_cast<unsigned long long>(te));
            for (uint32_t sb = 0; sb < 4; ++sb) if (tn[sb]) bn[sb] = rtk_atomic_add(rb.n_heavy.get() + 8 + sb, static_cast<unsigned long long>(tn[sb]));
        }
        bh = rtk_shfl(bh, 0); bl = rtk_shfl(bl, 0); be = rtk_shfl(be, 0); for (uint32_t sb = 0; sb < 4; ++sb) bn[sb] = rtk_shfl(bn[sb], 0);
        const uint64_t below = (1ull << rtk_lane()) - 1ull;
#pragma unroll
        for (int q = 0; q < RTK_OQ; ++q) {
            const uint64_t i = i0 + static_cast<uint64_t>(q) * RTK_WAVE + static_cast<uint64_t>(rtk_lane());
            const uint64_t mine = 1ull << rtk_lane();
            if (mh[q] & mine) rb.rorder[bh + static_cast<unsigned long long>(rtk_popc(mh[q] & below))] = static_cast<uint32_t>(i);
            else if (me[q] & mine) rb.eorder[be + static_cast<unsigned long long>(rtk_popc(me[q] & below))] = static_cast<uint32_t>(i);
            else if (ml[q] & mine) rb.rorder[n_regions - 1ull - (bl + static_cast<unsigned long long>(rtk_popc(ml[q] & below)))] = static_cast<uint32_t>(i);
            else for (uint32_t sb = 0; sb < 4; ++sb) if (mn[q][sb] & mine) rb.lorder[sb * rb.regions_cap + bn[sb] + static_cast<unsigned long long>(rtk_popc(mn[q][sb] & below))] = static_cast<uint32_t>(i);
            bh += static_cast<unsigned long long>(rtk_popc(mh[q])); bl += static_cast<unsigned long long>(rtk_popc(ml[q])); be += static_cast<unsigned long long>(rtk_popc(me[q])); for (uint32_t sb = 0; sb < 4; ++sb) bn[sb] += static_cast<unsigned long long>(rtk_popc(mn[q][sb]));
        }
    }
}

// The regions that need no graph walk, written straight into the segment pool: [read bases] + [bases of one unitig] and [top quality] + [bottom
// quality] (src/Correction.cpp:165-171 whole reads, :814-858 same-unitig shortcut, :920-932 uncorrected gap, :951-955 read end on a solid anchor).
// 64 regions per wave and round: one lane per region walks the descriptors (read, anchors, unitig: six dependent loads, 64 chains in flight), the
// lengths are summed across the wave and ONE atomic reserves the pool space of all 64 (same-address atomics retire at ~10 ns each: one per region
// was 3 ms per launch); then the wave writes the regions one after the other, 64 characters at a time.
struct RtkEasy { uint64_t src; uint64_t b0; uint32_t len_a, len_b, n_max, n_min, n_dec, strand; };
RTK_GLOBAL void k_regions_easy(const LaunchCtx* L, int grid) {
    const GraphView& g = L->g; const OptsView& o = L->o; const BatchView& bv = L->bv; const RegionBatch& rb = L->rb;
    const unsigned long long n_easy = rtk_u(rb.n_heavy[2]);
    const uint32_t k = static_cast<uint32_t>(g.k);
    const char q_min = rtk_get_qual(0.0, 0, static_cast<uint64_t>(o.max_qual)), q_max = rtk_get_qual(1.0, 0, static_cast<uint64_t>(o.max_qual));
    const char* const seq = bv.seq.get(); const uint64_t* const useq = g.useq.get(); char* const pool = rb.seg_pool.get();
    unsigned long long npb = 0;
    for (unsigned long long i0 = static_cast<unsigned long long>(RTK_BLOCK_ID) * RTK_WAVE; i0 < n_easy; i0 += static_cast<unsigned long long>(grid) * RTK_WAVE) {
        const unsigned long long i = i0 + static_cast<unsigned long long>(rtk_lane());
        const bool in = i < n_easy;
        RtkEasy e; e.src = 0; e.b0 = 0; e.len_a = 0; e.len_b = 0; e.n_max = 0; e.n_min = 0; e.n_dec = 0; e.strand = 1;
        RegionDesc* rd = nullptr;
        if (in) {
            rd = rb.regions.get() + rb.eorder[i];
            const uint32_t r = rd->read, kind = rd->kind;
            const uint64_t base = bv.roff[r]; const uint32_t Lr = static_cast<uint32_t>(bv.roff[r + 1] - base);
            if (kind == RTK_RG_WHOLE_MAX || kind == RTK_RG_WHOLE_MIN) { e.src = base; e.len_a = Lr; if (kind == RTK_RG_WHOLE_MAX) e.n_max = Lr; else e.n_min = Lr; }
            else if (kind == RTK_RG_TAIL_COPY) { const uint32_t prev_pos = rd->prev_pos, pa = bv.s_pos[base + rd->i_solid]; e.src = base + prev_pos; e.len_a = Lr - prev_pos; e.n_max = pa - prev_pos + k; e.n_min = Lr - pa - k; }
            else { // RTK_RG_GAP
                const uint32_t prev_pos = rd->prev_pos, pa = bv.s_pos[base + rd->i_solid], pb = bv.s_pos[base + rd->i_solid + 1];
                bool shortcut = false; UMap ua = rtk_um_empty(); uint32_t len_unitig_km = 0, min_pos = 0;
                (void)rtk_gap_is_easy(g, o, bv, *rd, &shortcut, &ua, &len_unitig_km, &min_pos);
                e.src = base + prev_pos;
                if (shortcut) { // the unitig between the anchors: the k-mers [min_pos, min_pos + len_unitig_km], all but the last k characters of their string
                    e.len_a = pa - prev_pos; e.len_b = len_unitig_km; e.n_dec = len_unitig_km + k; e.n_max = e.len_a + e.len_b;
                    e.b0 = g.uoff[ua.unitig] + min_pos; e.strand = ua.strand;
                } else {
                    e.len_a = pb - prev_pos;
                    if (pb < pa + k) e.n_max = (pa - prev_pos) + (pb - pa); else { e.n_max = (pa - prev_pos) + k; e.n_min = pb - pa - k; }
                }
            }
        }
        const uint32_t sl = e.len_a + e.len_b, ql = e.n_max + e.n_min;
        int total = 0; const int mine = rtk_wave_excl_scan(static_cast<int>(in ? sl + ql : 0u), &total);
        unsigned long long off0 = 0;
        if (rtk_lane() == 0 && total) off0 = rtk_atomic_add(rb.seg_top, static_cast<unsigned long long>(total));
        off0 = rtk_u(rtk_shfl(off0, 0));
        const unsigned long long off = off0 + static_cast<unsigned long long>(mine);
        if (in) { rd->seg_off = off; rd->seq_len = sl; rd->qual_len = ql; rd->status = 0; }
        if (off0 + static_cast<unsigned long long>(rtk_u(total)) > rb.seg_cap) continue; // (the host sees seg_top beyond seg_cap and reports it)
        const int cnt = static_cast<int>((n_easy - i0) < static_cast<unsigned long long>(RTK_WAVE) ? (n_easy - i0) : static_cast<unsigned long long>(RTK_WAVE));
        for (int j = 0; j < cnt; ++j) {
            const uint64_t src = rtk_u(rtk_shfl(e.src, j)), b0 = rtk_u(rtk_shfl(e.b0, j)); const unsigned long long o_j = rtk_u(rtk_shfl(off, j));
            const uint32_t len_a = rtk_u(rtk_shfl(e.len_a, j)), len_b = rtk_u(rtk_shfl(e.len_b, j)), n_max = rtk_u(rtk_shfl(e.n_max, j)), n_min = rtk_u(rtk_shfl(e.n_min, j)), n_dec = rtk_u(rtk_shfl(e.n_dec, j)), strand = rtk_u(rtk_shfl(e.strand, j));
            char* out = pool + o_j;
            for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < len_a; x += RTK_WAVE) out[x] = seq[src + x];
            for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < len_b; x += RTK_WAVE) { // mappedSequenceToString (as rtk_um_decode), first len_b characters
                const uint64_t pos = strand ? (b0 + x) : (b0 + (n_dec - 1 - x));
                const uint32_t bb = static_cast<uint32_t>((useq[pos >> 5] >> (2 * (pos & 31))) & 3ull);
                out[len_a + x] = static_cast<char>((0x54474341u >> (8 * (strand ? bb : (3u - bb)))) & 0xFFu);
            }
            const uint32_t sl_j = len_a + len_b, ql_j = n_max + n_min;
            for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < ql_j; x += RTK_WAVE) out[sl_j + x] = x < n_max ? q_max : q_min;
            npb += n_dec;
        }
    }
    if (rtk_lane() == 0 && npb) rtk_atomic_add(L->bv.counters + RTK_CNT_PATHBASE, npb);
}

// Lane-per-region kernel (rtk_region_lane.h): 64 regions of the lane class per wave and round, one per lane; persistent waves pull rounds of 64
// list entries from a device-wide counter. A lane that finishes its region parks its segment in its work area; at the end of the round the wave adds
// up the lengths, reserves the pool space of all 64 with ONE atomic and every lane copies its segment out. A region the lane program does not hold
// (status code != 0) is appended to the list of handed-on regions (horder), which the wave kernel takes when both kernels are through.
struct RlLimits { uint32_t str, um, list, arena0, arena1, arena2, tb; };
RTK_GLOBAL void k_regions_lanes(const LaunchCtx* L, uint32_t* area, uint64_t* table, uint64_t n_regions, RlLimits lim, int grid, int round_lanes) {
    const RegionBatch& rb = L->rb; const BatchView& bv = L->bv;
    (void)grid;
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
#ifndef RTK_SIM
    __builtin_amdgcn_s_setprio(3); // beside the wave kernel's persistent waves: a lane program is one long dependent chain, its wave goes first whenever it can issue
    const unsigned long long round = static_cast<unsigned long long>(round_lanes < 1 ? 1 : (round_lanes > RTK_WAVE ? RTK_WAVE : round_lanes)); // regions per wave and round (<= 64: fewer lanes per wave diverge less, more waves hide more latency)
#else
    const unsigned long long round = RTK_WAVE; (void)round_lanes;
#endif
    if (lane == 0) { // the wave-uniform context (LDS)
        RlEnv e;
        e.g = &L->g; e.o = &L->o; e.bv = &L->bv; e.rb = &L->rb;
        e.m = area + static_cast<uint64_t>(RTK_BLOCK_ID) * (static_cast<uint64_t>(RL_WORDS) * RL_STRIDE);
        e.tb = table + static_cast<uint64_t>(RTK_BLOCK_ID) * (static_cast<uint64_t>(RL_TB_WORDCOLS) * 2ull * RL_STRIDE);
        e.k = static_cast<uint32_t>(static_cast<int32_t>(L->g.k));
        e.lim_str = lim.str; e.lim_um = lim.um; e.lim_list = lim.list; e.lim_arena[0] = lim.arena0; e.lim_arena[1] = lim.arena1; e.lim_arena[2] = lim.arena2; e.lim_tb = lim.tb;
        rl_env = e;
    }
    rtk_sync();
    RlCtx c;
    c.c_expand = 0; c.c_colour = 0; c.c_pathbase = 0; c.c_align = 0; c.c_cells = 0;
    unsigned long long n_handed = 0, n_done = 0;
#ifdef RTK_LANE_PROF
    for (int x = 0; x < RL_NPROF; ++x) { c.prof[x] = 0; c.prof2[x] = 0; } c.prof_t = rtk_clock(); c.prof_cur = RL_P_DRIVER;
#endif
    for (int sub = 3; sub >= 0; --sub) { // the quarters of the class's gap range, the longest gaps first: the 64 regions of a round are of a size
    const unsigned long long n_lane = rtk_u(rb.n_heavy[8 + sub]);
    const uint32_t* const lorder = rb.lorder.get() + static_cast<uint64_t>(sub) * rb.regions_cap;
    while (true) {
        unsigned long long i0 = 0;
        if (lane == 0) i0 = rtk_atomic_add(rb.next_lane.get() + sub, round);
        i0 = rtk_u(rtk_shfl(i0, 0));
        if (i0 >= n_lane) break;
        const unsigned long long idx = i0 + lane;
        const bool in = idx < n_lane && lane < round;
        uint32_t osl = 0, oql = 0; RegionDesc* rd = nullptr;
        c.fail() = 0;
        if (in) {
            rd = rb.regions.get() + lorder[idx];
            c.top(0) = 0; c.top(1) = 0; c.top(2) = 0; c.memo_n() = 0; c.n_all() = 0; c.sv_valid = 0;
            const uint32_t e0 = c.c_expand, e1 = c.c_colour, e2 = c.c_pathbase, e3 = c.c_align; const unsigned long long e4 = c.c_cells;
#if defined(RTK_SIM) && defined(RTK_LANE_PROF)
            const unsigned long long tr0_ = rtk_clock();
#endif
            rl_region_program(c, rd, &osl, &oql);
#if defined(RTK_SIM) && defined(RTK_LANE_PROF)
            if (rtk_knob_lane_cost()) { const uint32_t* sp_ = bv.s_pos + bv.roff[rd->read]; fprintf(stderr, "LANECOST gap %u cycles %llu expand %u align %u cells %llu fail %u\n", sp_[rd->i_solid + 1] - sp_[rd->i_solid], rtk_clock() - tr0_, c.c_expand - e0, c.c_align - e3, c.c_cells - e4, c.fail()); }
#endif
            if (c.fail()) { osl = 0; oql = 0; c.c_expand = e0; c.c_colour = e1; c.c_pathbase = e2; c.c_align = e3; c.c_cells = e4; } // (the wave kernel counts the region's events when it redoes it)
        }
        RL_LAP(c, RL_P_DRIVER);
        int total = 0; const int mine = rtk_wave_excl_scan(static_cast<int>(osl + oql), &total);
        RL_LAP(c, RL_P_IDLE);
        unsigned long long off0 = 0;
        if (lane == 0 && total) off0 = rtk_atomic_add(rb.seg_top, static_cast<unsigned long long>(total));
        off0 = rtk_u(rtk_shfl(off0, 0));
        if (in) {
            if (c.fail()) { // handed on: the wave kernel finds it at the back of its light list
                rd->status = c.fail(); ++n_handed;
                const unsigned long long at = rtk_atomic_add(rb.n_heavy.get() + 4, 1ull);
                rb.horder[at] = lorder[idx];
            } else {
                const unsigned long long off = off0 + static_cast<unsigned long long>(mine);
                rd->seg_off = off; rd->seq_len = osl; rd->qual_len = oql; rd->status = 0; ++n_done;
                if (off + osl + oql <= rb.seg_cap) { // (beyond the pool: the host sees seg_top > seg_cap and reports it)
                    char* out = rb.seg_pool.get() + off;
                    for (uint32_t x = 0; x < osl; ++x) out[x] = static_cast<char>(rl_ldb(c, rl_sb(RL_SB_OUTS) + x));
                    for (uint32_t x = 0; x < oql; ++x) out[osl + x] = static_cast<char>(rl_ldb(c, rl_sb(RL_SB_OUTQ) + x));
                }
            }
        }
        RL_LAP(c, RL_P_EMIT);
    }
    }
#ifdef RTK_LANE_PROF
    { for (int x = 0; x < RL_NPROF; ++x) { unsigned long long v_ = c.prof[x], w_ = c.prof2[x];
#ifndef RTK_SIM
      for (int o = 32; o > 0; o >>= 1) { v_ += __shfl_xor(v_, o, 64); w_ += __shfl_xor(w_, o, 64); }
#endif
      if (lane == 0 && v_) { rtk_atomic_add(bv.counters + RTK_CNT_LANE_PROF + x, v_); rtk_atomic_add(bv.counters + RTK_CNT_LANE_PROF2 + x, w_); } } }
#endif
    {
    // event counters: one atomic per wave and counter
    unsigned long long v[7] = { c.c_expand, c.c_colour, c.c_pathbase, c.c_align, c.c_cells, n_handed, n_done };
#ifndef RTK_SIM
    for (int x = 0; x < 7; ++x) for (int o = 32; o > 0; o >>= 1) v[x] += __shfl_xor(v[x], o, 64);
#endif
    if (lane == 0) {
        if (v[0]) rtk_atomic_add(bv.counters + RTK_CNT_EXPAND, v[0]); if (v[1]) rtk_atomic_add(bv.counters + RTK_CNT_COLOUR, v[1]); if (v[2]) rtk_atomic_add(bv.counters + RTK_CNT_PATHBASE, v[2]);
        if (v[3]) rtk_atomic_add(bv.counters + RTK_CNT_ALIGN, v[3]); if (v[4]) rtk_atomic_add(bv.counters + RTK_CNT_CELLS, v[4]);
        if (v[5]) rtk_atomic_add(bv.counters + RTK_CNT_LANE_HANDED, v[5]); if (v[6]) rtk_atomic_add(bv.counters + RTK_CNT_LANE_DONE, v[6]); // lane kernel: regions handed on / done
    }
    }
}

// Persistent region kernel: each wave pulls the next region index from a device-wide counter until the list is drained
// (heavy-tailed per-region cost; see MI355X_MICROARCH "dequeue": ~0.3-1 us per pull). The pull for the NEXT region is issued before the
// current one is processed, so that its round trip (the counter, then rorder[]) hides behind the region's work.
#if defined(RTK_REGION_WPE) && !defined(RTK_SIM)
__attribute__((amdgpu_waves_per_eu(RTK_REGION_WPE, RTK_REGION_WPE))) // A/B knob: register budget of the region kernel (512 / waves per SIMD)
#endif
// which: 1 = the heavy and light lists (rorder), 2 = the regions the lane kernel handed on (horder), 3 = both (the redo launches)
RTK_GLOBAL void k_regions(const LaunchCtx* L, GraphView g, OptsView o, BatchView bv, RegionBatch rb, char* scratch, uint64_t stride, RegionScratchCfg cfg, uint64_t n_regions, int only_flagged, int trace_class, int which) {
#ifdef RTK_SIM
    RegionScratch hdr;
#else
    __shared__ RegionScratch hdr;
#endif
    RegionScratch* sc = region_scratch_carve(scratch + static_cast<uint64_t>(RTK_BLOCK_ID) * stride, cfg, &hdr);
    rtk_sync();
    (void)o;
    RCtx c = {L->g, L->o, L->bv, L->rb, {rtk_opaque(sc)}, {g.k}};
    const unsigned long long n_hv = (which & 1) ? rtk_u(rb.n_heavy[0]) : 0ull, n_lt = (which & 1) ? rtk_u(rb.n_heavy[1]) : 0ull; // the regions that are searched: heavy ones at the front of rorder[], light ones at its back
    const unsigned long long n_ho = (which & 2) ? rtk_u(rb.n_heavy[4]) : 0ull; // handed on by the lane kernel
    unsigned long long nxt = 0;
    if (rtk_lane() == 0) nxt = rtk_atomic_add(rb.next_region, 1ull);
#if !defined(RTK_SIM)
    // developer figures of a traced run (RTK_CNT_WAVE_TRACE): the longest single region, when the first wave started and the last one ended, the sum of the waves' lifetimes
    const unsigned long long wall0 = trace_class >= -1 ? 0ull : wall_clock64(); unsigned long long dt_max = 0, n_mine = 0, idx_of_max = 0;
#endif
    int steal_sub = 0; // which & 4: own lists drained, the regions of the lane kernel's class one at a time, from the queue that kernel takes its rounds of 64 from
    while (true) {
        const unsigned long long idx = rtk_u(rtk_shfl(nxt, 0));
        uint32_t ri; bool stolen = false;
        if (idx < n_hv + n_lt + n_ho) {
            ri = rtk_u(idx < n_hv + n_lt ? rb.rorder[idx < n_hv ? idx : (n_regions - n_lt) + (idx - n_hv)] : rb.horder[idx - n_hv - n_lt]);
            if (rtk_lane() == 0) nxt = rtk_atomic_add(rb.next_region, 1ull); // (consumed at the top of the next round)
        } else if ((which & 4) && steal_sub < 4) {
            ri = RTK_NONE32;
            while (steal_sub < 4) { // the quarters of the class from the shortest gaps up (the lane kernel starts from the longest)
                unsigned long long at = 0;
                if (rtk_lane() == 0) at = rtk_atomic_add(rb.next_lane.get() + steal_sub, 1ull);
                at = rtk_u(rtk_shfl(at, 0));
                if (at < rtk_u(rb.n_heavy[8 + steal_sub])) { ri = rtk_u(rb.lorder[static_cast<uint64_t>(steal_sub) * rb.regions_cap + at]); stolen = true; break; }
                ++steal_sub;
            }
            if (ri == RTK_NONE32) break;
        } else break;
        RegionDesc* rd = rb.regions + ri;
        if (only_flagged && rd->status == 0) continue;
        if (trace_class >= 0) { // developer runs (RTK_TRACE_CLASS): only the regions of one size class, so that the cycle shares are that class's (output is not valid)
            int hb = RTK_GAP_CLASS_HEAD_TAIL;
            if (rd->kind == RTK_RG_GAP) { const uint32_t* sp = bv.s_pos + bv.roff[rd->read]; const uint32_t gl = sp[rd->i_solid + 1] - sp[rd->i_solid]; hb = rtk_gap_class(gl); }
            if (hb != trace_class) continue;
        }
        *sc->overflow = 0; sc->top[RTK_ARENA_REGION] = 0; sc->top[RTK_ARENA_BFS] = 0; sc->top[RTK_ARENA_DFS] = 0; sc->memo_n = 0;
        RTK_PAIR_REGION();
#ifdef RTK_PROF
        { // in-situ latency probes (developer build): a chain of 4 dependent loads from random slots of the k-mer table (cold: HBM), one of 4 dependent
          // loads from the first words of the unitig offsets (warm: L2 / memory-side cache), one store + load of the wave's own slab
            const uint64_t* ht = reinterpret_cast<const uint64_t*>(g.ht.get()); const uint64_t nsl = g.ht_slots ? g.ht_slots : 1;
            uint64_t x = (idx * 0x9E3779B97F4A7C15ull) ^ (static_cast<uint64_t>(RTK_BLOCK_ID) << 20);
            unsigned long long t0_ = rtk_clock();
            for (int q = 0; q < 4; ++q) { x = rtk_u(ht[2ull * ((x >> 7) % nsl)]) + x * 0x9E3779B97F4A7C15ull + q; }
            unsigned long long t1_ = rtk_clock();
            uint64_t y = x & 7ull;
            for (int q = 0; q < 4; ++q) { y = (rtk_u(g.uoff[y & 63ull]) + y) & 63ull; }
            unsigned long long t2_ = rtk_clock();
            volatile uint64_t* slab = reinterpret_cast<volatile uint64_t*>(sc->str[RTK_STR_PROBE].get());
            slab[rtk_lane()] = y + x; const uint64_t z = slab[(rtk_lane() + 1) & 63];
            unsigned long long t3_ = rtk_clock() + (z & 1ull);
            sc->prof[RTK_LAP_PROBE_COLD] += t1_ - t0_; sc->prof[RTK_LAP_PROBE_WARM] += t2_ - t1_; sc->prof[RTK_LAP_PROBE_SLAB] += t3_ - t2_; sc->prof[RTK_LAP_PROBE_SAMPLES] += 1; sc->prof_t = rtk_clock();
        }
#endif
        const unsigned long long t0 = rtk_clock();
        const unsigned long long exp0 = RTK_HIST_GET(*sc, RTK_H_DFS_RUNNING);
        rtk_region_program(c, rd);
        { const unsigned long long dt = rtk_clock() - t0; sc->cnt[RTK_RC_CYC_TOTAL] += dt;
#if !defined(RTK_SIM)
          if (trace_class < -1) { ++n_mine; if (dt > dt_max) { dt_max = dt; idx_of_max = idx; } }
#endif
          int hb = RTK_GAP_CLASS_HEAD_TAIL;
          if (rd->kind == RTK_RG_GAP) { const uint32_t* sp = bv.s_pos + bv.roff[rd->read]; const uint32_t gl = sp[rd->i_solid + 1] - sp[rd->i_solid]; hb = rtk_gap_class(gl); }
          else if (rd->kind != RTK_RG_HEAD && rd->kind != RTK_RG_TAIL) hb = -1;
          if (hb >= 0) { RTK_HIST_ADD(*sc, RTK_H_CYCLES + hb, dt); RTK_HIST_ADD(*sc, RTK_H_REGIONS + hb, 1); RTK_HIST_ADD(*sc, RTK_H_DFS + hb, RTK_HIST_GET(*sc, RTK_H_DFS_RUNNING) - exp0); } } // (hb == RTK_GAP_CLASS_HEAD_TAIL: the last slot is RTK_H_DFS_RUNNING itself, see RtkHist)
        rd->status = *sc->overflow;
        if (*sc->overflow && rtk_lane() == 0) {
            rtk_atomic_add(rb.n_overflow, 1ull);
            // a region taken from the lane kernel's class is on neither list the redo launches walk (rorder, horder): it joins the handed-on ones
            if (stolen) { const unsigned long long at = rtk_atomic_add(rb.n_heavy.get() + 4, 1ull); rb.horder[at] = ri; }
        }
    }
#if !defined(RTK_SIM)
    if (trace_class < -1 && rtk_lane() == 0) {
        const unsigned long long wall1 = wall_clock64();
        atomicMax(reinterpret_cast<unsigned long long*>(bv.counters + RTK_CNT_WAVE_TRACE + 0), dt_max); atomicMax(reinterpret_cast<unsigned long long*>(bv.counters + RTK_CNT_WAVE_TRACE + 1), ~wall0); atomicMax(reinterpret_cast<unsigned long long*>(bv.counters + RTK_CNT_WAVE_TRACE + 2), wall1);
        rtk_atomic_add(bv.counters + RTK_CNT_WAVE_TRACE + 3, wall1 - wall0); rtk_atomic_add(bv.counters + RTK_CNT_WAVE_TRACE + 4, 1ull);
        if (dt_max > 0 && atomicMax(reinterpret_cast<unsigned long long*>(bv.counters + RTK_CNT_WAVE_TRACE + 5), dt_max) < dt_max) bv.counters[RTK_CNT_WAVE_TRACE + 6] = idx_of_max; // (racy on purpose: a hint of WHERE in the order the longest region sat)
        // when this wave took its last region off the queue, relative to the first start: waves that stop early leave their slots idle
        atomicMax(reinterpret_cast<unsigned long long*>(bv.counters + RTK_CNT_WAVE_TRACE + 7), n_mine);
    }
#endif
    if (rtk_lane() == 0) {
        rtk_atomic_add(bv.counters + RTK_CNT_EXPAND, sc->cnt[RTK_RC_EXPAND]); rtk_atomic_add(bv.counters + RTK_CNT_COLOUR, sc->cnt[RTK_RC_COLOUR]); rtk_atomic_add(bv.counters + RTK_CNT_PATHBASE, sc->cnt[RTK_RC_PATHBASE]);
        rtk_atomic_add(bv.counters + RTK_CNT_ALIGN, sc->cnt[RTK_RC_ALIGN]); rtk_atomic_add(bv.counters + RTK_CNT_CELLS, sc->cnt[RTK_RC_CELLS]);
        for (int i = 0; i < 6; ++i) rtk_atomic_add(bv.counters + RTK_CNT_CYC + i, sc->cnt[RTK_RC_CYC_COLOUR + i]);
        rtk_atomic_add(bv.counters + RTK_CNT_CYC_SETS, sc->cnt[RTK_RC_CYC_PATHREC]); rtk_atomic_add(bv.counters + RTK_CNT_CYC_TOSTRING, sc->cnt[RTK_RC_CYC_TOSTRING]); rtk_atomic_add(bv.counters + RTK_CNT_CYC_PATHQUAL, sc->cnt[RTK_RC_CYC_PATHQUAL]); rtk_atomic_add(bv.counters + RTK_CNT_WALK_CYCLES, sc->my.walk_cycles); rtk_atomic_add(bv.counters + RTK_CNT_WALK_MOVES, sc->my.walk_moves); rtk_atomic_add(bv.counters + RTK_CNT_WALK_RELOADS, sc->my.walk_reloads); rtk_atomic_add(bv.counters + RTK_CNT_WALK_SCALAR, sc->my.walk_scalar); rtk_atomic_add(bv.counters + RTK_CNT_WALK_CALLS, sc->my.walk_calls); rtk_atomic_add(bv.counters + RTK_CNT_WALK_TAIL, sc->my.walk_tail_cycles); rtk_atomic_add(bv.counters + RTK_CNT_CYC_DFS, sc->cnt[RTK_RC_CYC_DFS]); rtk_atomic_add(bv.counters + RTK_CNT_CYC_COLOUR_OK, sc->cnt[RTK_RC_CYC_COLOUR_OK]);
        for (int i = 0; i < RTK_FINE_N; ++i) rtk_atomic_add(bv.counters + RTK_CNT_FINE + i, sc->fine[i]);
        for (int i = RTK_RC_TRIM_STORED; i < RTK_RC_FA_LINKED_RUN; ++i) rtk_atomic_add(bv.counters + RTK_CNT_ROUTES + (i - RTK_RC_TRIM_STORED), sc->cnt[i]);
        for (int i = RTK_RC_FA_LINKED_RUN; i < RTK_RC_STRAND2_RUN; ++i) rtk_atomic_add(bv.counters + RTK_CNT_FA_LINKED + (i - RTK_RC_FA_LINKED_RUN), sc->cnt[i]);
        for (int i = RTK_RC_STRAND2_RUN; i < RTK_RC_PARK_WALKED; ++i) rtk_atomic_add(bv.counters + RTK_CNT_STRAND2 + (i - RTK_RC_STRAND2_RUN), sc->cnt[i]);
        for (int i = RTK_RC_PARK_WALKED; i < RTK_RC_COLOURS_SMALL; ++i) rtk_atomic_add(bv.counters + RTK_CNT_PARK + (i - RTK_RC_PARK_WALKED), sc->cnt[i]);
        for (int i = RTK_RC_COLOURS_SMALL; i < RTK_RC_PARK_RESWEEPS; ++i) rtk_atomic_add(bv.counters + RTK_CNT_COLOURS + (i - RTK_RC_COLOURS_SMALL), sc->cnt[i]);
        rtk_atomic_add(bv.counters + RTK_CNT_PARK_RESWEEPS, sc->cnt[RTK_RC_PARK_RESWEEPS]);
        for (int i = 0; i < RTK_H_N; ++i) rtk_atomic_add(bv.counters + RTK_CNT_HIST + i, static_cast<unsigned long long>(RTK_HIST_GET(*sc, i)));
#ifdef RTK_PROF
        for (int i = 0; i < RTK_LAP_N; ++i) rtk_atomic_add(bv.counters + RTK_CNT_PROF + i, static_cast<unsigned long long>(sc->prof[i]));
#endif
    }
}

RTK_GLOBAL void k_stitch(const LaunchCtx* L, BatchView bv, int grid) {
    for (uint32_t ri = static_cast<uint32_t>(RTK_BLOCK_ID); ri < bv.n_reads; ri += static_cast<uint32_t>(grid)) rtk_stitch_offsets(L->bv, L->rb, bv.order[ri]); // longest reads first
}
RTK_GLOBAL void k_stitch_copy(const LaunchCtx* L, uint64_t n_regions, int grid) {
    for (uint64_t c0 = static_cast<uint64_t>(RTK_BLOCK_ID) * RTK_WAVE; c0 < n_regions; c0 += static_cast<uint64_t>(grid) * RTK_WAVE) rtk_stitch_copy(L->rb, c0, n_regions);
}

static bool region_compact() { return rtk_knob_compact(); } // measured on configs[1]: same kernel time as the full-size areas (78.4 vs 79.5 ms) plus a 19 ms redo launch; kept for graphs that leave little HBM
// resident waves of the region stage whose work areas (`stride` bytes each) fit next to a big graph: at most 70 % of what is free now plus what the
// stage holds already (`held`); 4096 when there is room (a 5 Mb .. 60 Mb graph), never below 512
static int region_waves_that_fit(uint64_t stride, uint64_t held, bool trace) {
    int w = rtk_knob_region_waves();
#ifndef RTK_SIM
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && stride) {
        const uint64_t room = (static_cast<uint64_t>(fr) + held) / 10 * 7;
        if (trace) fprintf(stderr, "[rtk trace] region work areas: %.1f GB free + %.1f GB held of %.1f GB, %d waves x %.1f MB wanted\n", fr / 1073741824.0, held / 1073741824.0, tot / 1073741824.0, w, stride / 1048576.0);
        if (static_cast<uint64_t>(w) * stride > room) { uint64_t f = room / stride / 256 * 256; if (f < 512) f = 512; if (f < static_cast<uint64_t>(w)) w = static_cast<int>(f); }
    }
#else
    (void)stride; (void)held; (void)trace;
#endif
    return w;
}

static RegionScratchCfg region_cfg(uint32_t max_len_exact, int attempt) { // (declared in rtk_pipeline.inc for the phasing step)
    RegionScratchCfg c;
    uint32_t max_len = 131072u; while (max_len < max_len_exact) max_len <<= 1; // coarse steps: the per-wave slab (and the cached tens of GB behind it) keeps its size from batch to batch
    if (attempt == 0 && rtk_knob_test_tiny_scratch()) { // test hook: start from a deliberately undersized work area so that the redo path runs
        c.str_cap = 2048; c.my.w_cap = c.str_cap / 64 + 2; c.my.t_cap = c.str_cap; c.my.r_cap = c.str_cap; c.my.mv_cap = 2 * c.str_cap;
        c.my.tb_cap_words = 4ull * 52429 + 64; c.set_cap = 64; c.um_cap = 8; c.list_cap = 64; c.memo_cap = 16; c.bm_words = max_len / 64 + 8; c.arena_cap = 8192;
        return c;
    }
    // First attempt: a COMPACT work area sized for the regions that make up the bulk of a batch (weak regions are <= -w 1000 + k
    // characters, their paths a few kb): ~1.3 MB per wave instead of ~10 MB, so the 4096 resident waves touch ~5 GB instead of 41 GB of
    // HBM (address translation and the memory-side cache work on a working set 8x smaller). Anything bigger -- long uncorrectable
    // heads / tails copied through, huge sub-paths -- reports an overflow and is redone by the next attempt with the full-size areas.
    if (region_compact()) {
        if (attempt == 0) {
            c.str_cap = 65536; c.my.w_cap = c.str_cap / 64 + 2; c.my.t_cap = c.str_cap; c.my.r_cap = c.str_cap; c.my.mv_cap = 2 * c.str_cap;
            c.my.tb_cap_words = 4ull * 8192 + 64; c.set_cap = 4096; c.um_cap = 512; c.list_cap = 1024; c.memo_cap = 512; c.bm_words = c.str_cap / 64 + 8; c.arena_cap = 128u << 10;
            return c;
        }
        attempt -= 1;
    }
    const uint32_t scale = 1u << (3 * attempt); // 1, 8, 64
    c.str_cap = std::max<uint32_t>(65536u, (5u * max_len) / 2u + 1024u) * scale;
    c.my.w_cap = c.str_cap / 64 + 2; c.my.t_cap = c.str_cap; c.my.r_cap = c.str_cap; c.my.mv_cap = 2 * c.str_cap;
    c.my.tb_cap_words = std::max<uint64_t>(4ull * 52429 + 64, 4ull * c.my.w_cap + 64);
    c.set_cap = 16384u * scale; c.um_cap = 2048u * scale; c.list_cap = 4096u * scale; c.memo_cap = 2048u * scale;
    c.bm_words = max_len / 64 + 8; c.arena_cap = (1ull << 20) * scale;
    return c;
}

static int batch_precheck(rtk_batch* b, const rtk_opts* opts, const char* who) {
    if (!b || !opts) return rtk_fail(RTK_ERR_ARG, std::string(who) + ": null argument");
    if (!opts_ok(opts)) return rtk_fail(RTK_ERR_ARG, std::string(who) + ": rtk_opts was not filled by this library's rtk_opts_default (struct_size does not match: older header, or a zero-filled struct)");
    if (!b->g->on_device) return rtk_fail(RTK_ERR_NO_DEVICE, std::string(who) + ": graph is not resident on a device");
    return RTK_OK;
}

// stage A: anchors of every read (exact scan, mask, inexact scan, filters) on the batch's stream
extern "C" int rtk_batch_run_seeds(rtk_batch* b, const rtk_opts* opts) {
    int rc = batch_precheck(b, opts, "rtk_batch_run_seeds");
    if (rc) return rc;
    if (b->g->info.k > 31 && !opts->long_read_correct) return rtk_fail(RTK_ERR_ARG, "rtk_batch_run_seeds: graphs with k > 31 serve the second pass only (long_read_correct = 1): the 1-edit anchor search of the first pass is built for one-word k-mers");
    try {
        rtk_set_device(b->g->device);
        b->seeded = false; b->ran = false;
        b->t_all.start(b->stream);
        if (opts->long_read_correct && opts->force_unres_snp_corr && !b->snps_fixed) fix_snps_step(b); // fixSNPs() precedes phasing() (src/Ratatosk.cpp:828)
        if (opts->long_read_correct && b->has_raw && !b->phased) { rc = phase_step(b, opts_view(opts)); if (rc) return rc; } // phasing() precedes getSeeds (src/Ratatosk.cpp:832-838)
        rc = seed_stage_checked(b, opts_view(opts));
        if (rc == RTK_OK) b->seeded = true;
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return rc;
}

// ---- stage B, host side. rtk_batch_run_regions (below) calls these steps in order; what they hand on to each other lives in RegionRun.
// the graph-wide work areas of the region stage (rtk_graph::region_slab_take): one half (what = 0 / 1) or both (2), given back when the stage leaves
struct SlabHold {
    rtk_graph* g; int what;
    void take(bool half_ok) { what = g->region_slab_take(half_ok); }
    void release() { if (what >= 0) { g->region_slab_give(what); what = -1; } }
    ~SlabHold() { release(); }
};
// second pass: a work area of the ticket's own (no graph-wide lock, so that the tickets in flight overlap)
struct OwnSlab {
    rtk_graph* g; void* p; uint64_t n;
    char* at_least(uint64_t bytes) { if (n < bytes) { if (p) { g->phase_give(p, n); p = nullptr; n = 0; } p = g->phase_take(bytes, &n); } return static_cast<char*>(p); }
    ~OwnSlab() { if (p) g->phase_give(p, n); }
};
struct RegionRun {
    rtk_batch* b; rtk_graph* g; OptsView ov; rtk_stream_t sm;
    bool trace;     // RTK_TRACE, read once per call
    // Second pass: a ticket has few, big regions (one per 3 kb of read, up to -W 5000 characters) and its launch lasts as long as its
    // biggest one with most wave slots idle: it gets a work area of its own so that the tickets in flight overlap.
    bool own_slab;
    std::chrono::steady_clock::time_point w0;
    int grid; uint32_t max_len; unsigned long long n_regions, n_ovf_total, out_top;
    bool lane_auto, lanes_on, lanes_beside; int lane_waves_used;
    RtkTimer t_enum, t_easy, t_lanes, t_reg, t_st; double ms_reg;
    SlabHold hold; OwnSlab slab;
    const LaunchCtx* ctx() const { return static_cast<const LaunchCtx*>(b->ctx()); }
    void set_ctx() { rtk_launch(k_set_ctx, 1, sm, b->ctx(), g->dview, ov, b->bv, b->rb); }
    void lap(const char* what) const {
        if (trace) fprintf(stderr, "[rtk trace] regions %-10s +%.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count());
    }
};

// the lists that hold one entry per region
static void region_alloc_lists(rtk_batch* b, uint64_t cap) {
    RegionBatch& rb = b->rb;
    rb.regions_cap = cap;
    rb.regions = b->alloc<RegionDesc>(cap); rb.rorder = b->alloc<uint32_t>(cap); rb.eorder = b->alloc<uint32_t>(cap);
    rb.lorder = b->alloc<uint32_t>(4 * cap); rb.horder = b->alloc<uint32_t>(cap); rb.st_off = b->alloc<uint64_t>(cap);
}

// the per-batch buffers of the stage (first run of this batch only)
static void region_alloc(RegionRun& R) {
    rtk_batch* b = R.b; RegionBatch& rb = b->rb;
    if (rb.seq_rc) return;
    rb.seq_rc = b->alloc<char>(b->n_bases + 64);
    rb.qual_rev = b->bv.qual.get() ? b->alloc<char>(b->n_bases + 64) : nullptr;
    rb.r_first = b->alloc<uint64_t>(b->n); rb.r_count = b->alloc<uint32_t>(b->n);
    rb.n_regions = b->alloc<unsigned long long>(1); rb.n_heavy = b->alloc<unsigned long long>(16); rb.seg_top = b->alloc<unsigned long long>(1);
    rb.next_region = b->alloc<unsigned long long>(1); rb.n_overflow = b->alloc<unsigned long long>(1); rb.out_top = b->alloc<unsigned long long>(1);
    rb.out_off = b->alloc<uint64_t>(b->n); rb.out_seq_len = b->alloc<uint32_t>(b->n); rb.out_qual_len = b->alloc<uint32_t>(b->n);
    region_alloc_lists(b, std::max<uint64_t>(1024, b->n_bases / 8 + 4ull * b->n));
    rb.next_lane = b->alloc<unsigned long long>(4);
    rb.seg_cap = 6 * b->n_bases + (1ull << 20); rb.seg_pool = b->alloc<char>(rb.seg_cap);
    rb.out_cap = 6 * b->n_bases + (1ull << 20); rb.out_pool = b->alloc<char>(rb.out_cap);
}

// Which regions the lane-per-region kernel gets (known before the views go to the device): gaps under RTK_LANE_MAX_GAP bases (0 = off); none in the second pass.
// Off by default: the kernel is byte-identical to the wave kernel on every tier but not yet faster -- a lane's program is one long dependent chain, ~5 ms per
// region on one lane (DESIGN_HISTORY.md section 3.8) -- so a run opts in with RTK_LANE_MAX_GAP=128 (the bench measures both ways and reports the pair).
// It pays from ~10^6 lane-class regions per launch upwards (break-even at 253 Mb per ticket, -5.5 % of the region stage at
// 989 Mb, one kernel after the other on 4 096 lane waves: DESIGN_HISTORY.md section 3.8), so a ticket of at least RTK_LANE_AUTO_BASES (512 Mi; 0 = never) bases -- `Ratatosk correct -B`
// that large, or a caller's own -- takes it for gaps under 128 without being asked; smaller tickets (every ticket of the bench and of the CLI's default -B) never do.
static void region_lane_class(RegionRun& R) {
    const uint64_t auto_bases = rtk_knob_lane_auto_bases();
    R.lane_auto = !R.own_slab && !rtk_knob_lane_max_gap_set() && auto_bases != 0 && R.b->n_bases >= auto_bases;
    R.b->rb.lane_max_gap = R.own_slab ? 0u : (R.lane_auto ? 128u : rtk_knob_lane_max_gap());
}

// the regions of every read (k_enum; once more with bigger lists if there are more than expected), then their dequeue order: heavy regions first
static void region_enumerate(RegionRun& R) {
    rtk_batch* b = R.b; RegionBatch& rb = b->rb; const rtk_stream_t sm = R.sm;
    const int eg = std::min<int>(R.grid, static_cast<int>(b->n) > 0 ? static_cast<int>(b->n) : 1);
    for (int tries = 0; tries < 2; ++tries) {
        rtk_dzero_s(rb.n_regions, 8, sm);
        R.set_ctx();
        R.t_enum.start(sm);
        rtk_launch(k_enum, eg, sm, R.ctx(), b->bv, eg);
        R.t_enum.stop(sm);
        rtk_ssync(sm);
        rtk_d2h_s(&R.n_regions, rb.n_regions, 8, sm);
        if (R.n_regions <= rb.regions_cap) break;
        region_alloc_lists(b, R.n_regions + 1024);
    }
    if (R.n_regions) {
        rtk_dzero_s(rb.n_heavy, 128, sm);
        R.set_ctx();
        const unsigned long long per_wave = RTK_OQ * RTK_WAVE;
        const int og = static_cast<int>(std::min<unsigned long long>(static_cast<unsigned long long>(R.grid), (R.n_regions + per_wave - 1ull) / per_wave));
        rtk_launch(k_region_order, og, sm, R.ctx(), static_cast<uint64_t>(R.n_regions), og);
    }
}

// the regions without a graph walk (first pass): written by a light kernel of their own, 8 waves per SIMD
static void region_easy(RegionRun& R) {
    rtk_dzero_s(R.b->rb.seg_top, 8, R.sm); rtk_dzero_s(R.b->rb.out_top, 8, R.sm);
    if (!R.n_regions) return;
    const int eg = static_cast<int>(std::min<unsigned long long>(static_cast<unsigned long long>(2 * R.grid), R.n_regions));
    R.t_easy.start(R.sm);
    rtk_launch(k_regions_easy, eg, R.sm, R.ctx(), eg);
    R.t_easy.stop(R.sm);
}

// The light class, one region per lane (rtk_region_lane.h), on the batch's second stream BESIDE the wave kernel: its waves are few (64 regions each) and
// bound by the latency of one lane's program, the wave kernel's persistent waves fill the rest of the machine. What it hands on is taken by a second
// launch of the wave kernel when both are through. RTK_LANE_SERIAL=1: one after the other on the batch's stream (A/B).
static void region_lanes(RegionRun& R) {
    rtk_batch* b = R.b; RegionBatch& rb = b->rb; const rtk_stream_t sm = R.sm;
    R.lane_waves_used = 0;
    R.lanes_on = R.n_regions && rb.lane_max_gap;
    R.lanes_beside = R.lanes_on && !R.lane_auto && !rtk_knob_lane_serial();
    if (!R.lanes_on) return;
    R.hold.take(false); // (the lane kernel's areas, slot 2, belong to whoever holds both halves of slot 1)
#ifdef RTK_SIM
    const int lgrid = 16;
#else
    const int lgrid = R.lane_auto ? 4096 : rtk_knob_lane_waves();
#endif
    R.lane_waves_used = lgrid;
    const uint64_t a_bytes = rl_area_bytes(), t_bytes = rl_table_bytes();
    char* ls = graph_scratch(R.g, 2, (a_bytes + t_bytes) * static_cast<uint64_t>(lgrid));
    RlLimits lim;
    lim.str = RL_STR_BYTES; lim.um = RL_UM_CAP; lim.list = RL_LIST_CAP; lim.arena0 = RL_A0_W; lim.arena1 = RL_A1_W; lim.arena2 = RL_A2_W; lim.tb = RL_TB_WORDCOLS;
    if (rtk_knob_test_tiny_scratch()) { lim.str = 200; lim.um = 6; lim.list = 3; lim.arena0 = 160; lim.arena1 = 400; lim.arena2 = 400; lim.tb = 400; } // (most are handed on)
    rtk_dzero_s(rb.next_lane, 32, sm);
    rtk_stream_t sl = sm;
    if (R.lanes_beside) { sl = b->lane_stream(); rtk_event_record(b->ev[0], sm); rtk_stream_wait(sl, b->ev[0]); }
    R.t_lanes.start(sl);
    rtk_launch(k_regions_lanes, lgrid, sl, R.ctx(), reinterpret_cast<uint32_t*>(ls), reinterpret_cast<uint64_t*>(ls + a_bytes * static_cast<uint64_t>(lgrid)),
               static_cast<uint64_t>(R.n_regions), lim, lgrid, rtk_knob_lane_round());
    R.t_lanes.stop(sl);
    if (R.lanes_beside) rtk_event_record(b->ev[1], sl);
}

// The graph-wide work areas are taken here, not at the top: enumeration, ordering and the regions without a walk of one ticket run beside the region
// kernel of another. Tickets up to RTK_HALF_SLAB_BASES share them two at a time: above ~8 Mi a launch fills the 4 096 wave slots by itself (at 24 Mi a
// 16.8 Mb group took 18.9 ms on its half against 10-11 ms on both, profiles/r06_coalesce_trace.txt).
static void region_take_areas(RegionRun& R) {
    rtk_batch* b = R.b; rtk_graph* g = R.g;
    if (!R.own_slab && R.hold.what < 0) {
        const uint64_t half_max_bases = rtk_knob_half_slab_bases();
        R.hold.take(half_max_bases != 0 && b->n_bases <= half_max_bases && !region_compact());
        if (R.hold.what != 2) { // a half: only if the areas exist and half of them holds a useful number of waves of this ticket's size class; otherwise both after all
            const uint64_t st0 = region_scratch_bytes(region_cfg(R.max_len, 0)), half_bytes = (g->scratch_bytes_[1] / 2) & ~255ull;
            if (!g->scratch[1] || half_bytes / st0 < 512) { R.hold.release(); R.hold.take(false); }
        }
    }
    if (b->on_region_slab) { b->on_region_slab(b->on_region_slab_arg); b->on_region_slab = nullptr; }
}

// Waves of one launch of k_regions, from plain values. 128 VGPRs -> 4 waves/SIMD -> 16 single-wave workgroups per CU.
struct RegionGridIn {
    int attempt; bool compact;          // attempt 0 or a redo launch (compact: attempt 0 ran on compact areas, the full-size ones start at attempt 1)
    int waves_that_fit;                 // attempt 0: region_waves_that_fit
    bool own_slab; int p2_cap;          // second pass: RTK_P2_RGRID
    bool lanes_beside; int lane_waves;  // the lane kernel runs beside attempt 0 on that many waves
    bool on_half; int half_waves; uint64_t half_fit; // one half of the work areas: RTK_HALF_WAVES, and the waves whose areas fit into it
    unsigned long long n_regions;
};
static int region_grid(const RegionGridIn& in) {
#ifdef RTK_SIM
    int rgrid = 16;
#else
    const int big = in.attempt - (in.compact ? 1 : 0); // < 0: compact areas; 0, 1, 2: full-size areas x1, x8, x64
    int rgrid = in.attempt == 0 ? in.waves_that_fit : (big == 0 ? 1024 : (big == 1 ? 256 : 8));
#endif
    if (in.own_slab && in.attempt == 0)
        rgrid = static_cast<int>(std::min<unsigned long long>(static_cast<unsigned long long>(in.p2_cap), std::max<unsigned long long>(128ull, in.n_regions / 4ull)));
    // the lane kernel's waves need their slots from the start: the persistent waves of this kernel only leave at the end
    if (in.attempt == 0 && in.lanes_beside) rgrid = std::max(1024, rgrid - in.lane_waves);
    rgrid = static_cast<int>(std::min<unsigned long long>(static_cast<unsigned long long>(rgrid), in.n_regions ? in.n_regions : 1ull));
    // (measured: 1 536 / 1 024 waves per half, to leave the seed kernels of the ticket behind them wave slots, lose 4-20 %: profiles/r06_half_waves.txt)
    if (in.on_half) rgrid = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(std::min(rgrid, in.half_waves)), in.half_fit));
    return rgrid;
}

// which capacity the flagged regions ran out of (status codes of rtk_fail_ovf, by number: RtkOvf in rtk_region_types.h -- 1, 2 alignment, 3 arena, 4 .. 6 working path,
// 7 string, 8 list, 9 set, 10 bitmap, 11 SNP annotations / consensus stall, 12 segment pool, 14 fixRepeats), and the wave figures of a traced launch
static void region_attempt_trace(RegionRun& R, int attempt, int rgrid, uint64_t stride) {
    const BatchView& bv = R.b->bv; const rtk_stream_t sm = R.sm;
    std::vector<RegionDesc> rds(R.n_regions); rtk_d2h_s(rds.data(), R.b->rb.regions, sizeof(RegionDesc) * R.n_regions, sm);
    unsigned long long hist[16] = {0}; for (size_t i = 0; i < rds.size(); ++i) hist[rds[i].status & 15u]++;
    fprintf(stderr, "[rtk trace] k_regions attempt %d: %.2f ms, %d waves, stride %.2f MB; status codes:", attempt, R.t_reg.elapsed(), rgrid, stride / 1048576.0);
    for (int i = 1; i < 16; ++i) if (hist[i]) fprintf(stderr, " %d:%llu", i, hist[i]);
    fprintf(stderr, "\n");
    unsigned long long tc[RTK_CNT_WAVE_TRACE_END - RTK_CNT_WAVE_TRACE] = {0}; rtk_d2h_s(tc, bv.counters + RTK_CNT_WAVE_TRACE, sizeof(tc), sm);
    const double span = static_cast<double>(tc[2] - ~tc[1]) / 100e6 * 1e3, avg_life = tc[4] ? static_cast<double>(tc[3]) / static_cast<double>(tc[4]) / 100e6 * 1e3 : 0.0;
    fprintf(stderr, "[rtk trace] k_regions waves: first start to last end %.2f ms, average lifetime of a wave %.2f ms (%.0f %% of it), longest single region %.3g cycles "
                    "(taken off the queue at place %llu of %llu), most regions on one wave %llu\n",
            span, avg_life, span > 0 ? 100.0 * avg_life / span : 0.0, static_cast<double>(tc[0]), tc[6], static_cast<unsigned long long>(R.n_regions), tc[7]);
}

// k_regions until no region reports an overflow: any region that ran out of scratch is redone with a bigger arena (still on the device)
static int region_attempts(RegionRun& R) {
    rtk_batch* b = R.b; rtk_graph* g = R.g; RegionBatch& rb = b->rb; const rtk_stream_t sm = R.sm;
    const int n_attempts = region_compact() ? 4 : 3;
    R.ms_reg = 0; R.n_ovf_total = 0;
    for (int attempt = 0; attempt < n_attempts; ++attempt) {
        if (attempt != 0 && !R.own_slab && R.hold.what != 2) { R.hold.release(); R.hold.take(false); } // the redo launches may grow the areas: both halves
        const RegionScratchCfg cfg = region_cfg(R.max_len, attempt);
        const uint64_t stride = region_scratch_bytes(cfg);
        if (R.trace) fprintf(stderr, "[rtk trace] region work area: %llu bytes per wave\n", static_cast<unsigned long long>(stride));
        const bool on_half = !R.own_slab && R.hold.what != 2;
        const uint64_t half_bytes = (g->scratch_bytes_[1] / 2) & ~255ull;
        RegionGridIn gi;
        gi.attempt = attempt; gi.compact = region_compact(); gi.n_regions = R.n_regions;
#ifdef RTK_SIM
        gi.waves_that_fit = 0;
#else
        gi.waves_that_fit = attempt == 0 ? region_waves_that_fit(stride, R.own_slab ? 0 : g->scratch_bytes_[1], R.trace) : 0;
#endif
        gi.own_slab = R.own_slab; gi.p2_cap = rtk_knob_p2_rgrid();
        gi.lanes_beside = R.lanes_beside; gi.lane_waves = R.lane_waves_used;
        gi.on_half = on_half; gi.half_waves = on_half ? rtk_knob_half_waves() : 0; gi.half_fit = on_half ? half_bytes / stride : 0;
        const int rgrid = region_grid(gi);
        char* scratch;
        if (R.own_slab) scratch = R.slab.at_least(stride * rgrid);
        else if (!on_half) scratch = graph_scratch(g, 1, stride * rgrid);
        else scratch = static_cast<char*>(g->scratch[1]) + static_cast<uint64_t>(R.hold.what) * half_bytes;
        rtk_dzero_s(rb.next_region, 8, sm); rtk_dzero_s(rb.n_overflow, 8, sm);
        if (attempt != 0) R.set_ctx(); // (attempt 0: the views are in place since the order kernel, and the lane kernel may be reading them)
        const int tcls = rtk_knob_trace_class(R.trace ? -2 : -1);
        R.t_reg.start(sm);
        rtk_launch(k_regions, rgrid, sm, R.ctx(), g->dview, R.ov, b->bv, rb, scratch, stride, cfg, static_cast<uint64_t>(R.n_regions), attempt == 0 ? 0 : 1, tcls,
                   attempt == 0 ? (R.lanes_beside ? 5 : 1) : 3);
        if (attempt == 0 && R.lanes_on) { // the regions the lane kernel handed on
            if (R.lanes_beside) rtk_stream_wait(sm, b->ev[1]);
            rtk_dzero_s(rb.next_region, 8, sm);
            rtk_launch(k_regions, std::min(rgrid, 1024), sm, R.ctx(), g->dview, R.ov, b->bv, rb, scratch, stride, cfg, static_cast<uint64_t>(R.n_regions), 0, tcls, 2);
        }
        R.t_reg.stop(sm);
        rtk_ssync(sm);
        R.ms_reg += R.t_reg.elapsed();
        if (R.trace) region_attempt_trace(R, attempt, rgrid, stride);
        unsigned long long n_ovf = 0; rtk_d2h_s(&n_ovf, rb.n_overflow, 8, sm);
        if (attempt == 0) R.n_ovf_total = n_ovf;
        // the kernels that reserve pool space past the end skip their copies and raise nothing else (k_regions_easy, k_regions_lanes): looked at after EVERY attempt
        unsigned long long seg_top = 0; rtk_d2h_s(&seg_top, rb.seg_top, 8, sm);
        if (seg_top > rb.seg_cap) return rtk_fail(RTK_ERR_DEVICE, "region stage: segment pool exhausted");
        if (n_ovf == 0) return RTK_OK;
    }
    return rtk_fail(RTK_ERR_DEVICE, "region stage: scratch capacity exceeded after " + std::to_string(n_attempts) + " attempts");
}

// the corrected reads put together from their regions' segments; ends the stage's clock
static int region_stitch(RegionRun& R) {
    rtk_batch* b = R.b; const rtk_stream_t sm = R.sm;
    R.t_st.start(sm);
    const int sg = std::min<int>(R.grid, static_cast<int>(b->n) > 0 ? static_cast<int>(b->n) : 1);
    rtk_launch(k_stitch, sg, sm, R.ctx(), b->bv, sg);
    if (R.n_regions) {
        const int cg = static_cast<int>(std::min<unsigned long long>(static_cast<unsigned long long>(2 * R.grid), (R.n_regions + RTK_WAVE - 1ull) / RTK_WAVE));
        rtk_launch(k_stitch_copy, cg, sm, R.ctx(), static_cast<uint64_t>(R.n_regions), cg);
    }
    R.t_st.stop(sm);
    b->t_all.stop(sm);
    rtk_ssync(sm);
    R.out_top = 0; rtk_d2h_s(&R.out_top, b->rb.out_top, 8, sm);
    if (R.out_top > b->rb.out_cap) return rtk_fail(RTK_ERR_DEVICE, "stitch: output pool exhausted");
    return RTK_OK;
}

// everything that only RTK_TRACE prints at the end of the stage, from the copied counter block
static void region_trace_report(const unsigned long long* cnt) {
    const double total = double(cnt[RTK_CNT_CYC_TOTAL] ? cnt[RTK_CNT_CYC_TOTAL] : 1);
    auto share = [&](int slot) { return double(cnt[slot]) / total; };
#ifdef RTK_PROF
    {
        static const char* const pn[RTK_LAP_N] = { // by slot number: RtkLap
            "driver: dispatch + anchors", "driver: same-unitig shortcut", "region: prologue", "region: side lists", "region: chooseColors",
            "semiweak: glue", "paths: prologue", "explore: prefix", "dfs: pop + adj", "dfs: nkm + colour_ok", "dfs T: load/extend",
            "dfs T: to_string", "dfs T: NW sweep", "dfs T: commit", "dfs NT: load/extend", "dfs NT: commit/rest", "dfs post: nt scoring",
            "dfs post: load + to_string", "dfs post: path qual", "dfs post: commit", "paths: after explore", "paths: final select",
            "semiweak: merge", "region: restart/select", "region: assemble", "region: fixAmbiguity", "region: corrected? + trim",
            "driver: between fw/bw", "consensus: rc + card", "consensus: fw NW path", "consensus: bw path / checks", "consensus: merge",
            "consensus: final", "driver: emit prep", "dequeue", "emit", 0, 0, 0, 0, "probe: 4 dependent cold loads", "probe: 4 dependent warm loads",
            "probe: slab store + load", 0};
        const unsigned long long* pr = cnt + RTK_CNT_PROF; const int n = RTK_LAP_N;
        if (pr[RTK_LAP_PROBE_SAMPLES]) fprintf(stderr, "[rtk trace] in-situ probes: cold load %.0f cycles, warm load %.0f cycles, slab store + load %.0f cycles "
                                    "(per round trip, %llu samples)\n",
                            double(pr[RTK_LAP_PROBE_COLD]) / 4.0 / double(pr[RTK_LAP_PROBE_SAMPLES]), double(pr[RTK_LAP_PROBE_WARM]) / 4.0 / double(pr[RTK_LAP_PROBE_SAMPLES]), double(pr[RTK_LAP_PROBE_SLAB]) / double(pr[RTK_LAP_PROBE_SAMPLES]), pr[RTK_LAP_PROBE_SAMPLES]);
        unsigned long long tot = 0; for (int i = 0; i < n; ++i) tot += pr[i];
        fprintf(stderr, "[rtk trace] k_regions lap profile (%.3g cycles):", double(tot));
        for (int i = 0; i < n; ++i) if (pr[i] && pn[i]) fprintf(stderr, " [%d %s %.4f]", i, pn[i], double(pr[i]) / double(tot ? tot : 1));
        fprintf(stderr, "\n");
    }
#endif
    {
        static const char* const hn[RTK_GAP_CLASSES] = {"gap<40", "gap<64", "gap<128", "gap<256", "gap<512", "gap<1024", "gap>=1024", "head/tail"};
        const unsigned long long* h = cnt + RTK_CNT_HIST; // RegionScratch::hist (RtkHist)
        fprintf(stderr, "[rtk trace] k_regions by size class (share of region time, regions, avg kcycles, second-strand share, DFS calls per region):");
        for (int i = 0; i < RTK_GAP_CLASSES; ++i) {
            const unsigned long long cyc = h[RTK_H_CYCLES + i], n = h[RTK_H_REGIONS + i];
            if (n) fprintf(stderr, " [%s %.3f n=%llu %.0fk bw=%.2f dfs=%.1f]", hn[i], double(cyc) / total, n, 1e-3 * double(cyc) / double(n), double(h[RTK_H_STRAND2 + i]) / double(n),
                           double(h[RTK_H_DFS + i]) / double(n));
        }
        fprintf(stderr, "\n");
    }
    {
        static const char* const fine_names[RTK_FINE_N] = {
            "colour: class unions", "fixAmbiguity: path alignment", "fixAmbiguity: walk of the moves",
            "fixAmbiguity: linked alleles (k-mer lookups)", "fixAmbiguity: apply", "colour small: bit vectors (or array: shared_with(all))",
            "colour small: classes + selection (or array: set ops)", "region: side lists", "region: trim alignment", "region: fixAmbiguity",
            "consensus: merge logic", "paths: explore_paths outside DFS", "colour: small path (cycles)", "colour: 4096-bit path (cycles)",
            "colour: small path calls / total cycles", "colour: 4096-bit path calls / total cycles"};
        const unsigned long long* f = cnt + RTK_CNT_FINE;
        fprintf(stderr, "[rtk trace] chooseColors calls: small path %llu, 4096-bit path %llu; fixAmbiguity calls %llu, of which left by the all-confident way out %llu\n",
                f[RTK_FINE_COL_S_CALLS], f[RTK_FINE_COL_B_CALLS], f[RTK_FINE_FA_CALLS], f[RTK_FINE_FA_ALL_CONFIDENT]);
        fprintf(stderr, "[rtk trace] k_regions fine shares:");
        for (int i = 0; i < RTK_FINE_N; ++i) if (f[i]) fprintf(stderr, " [%s %.3f]", fine_names[i], double(f[i]) / total);
        fprintf(stderr, "\n");
    }
#ifdef RTK_LANE_PROF
    {
        static const char* const ln[RL_NPROF] = {
            "driver", "side lists", "chooseColors", "search glue", "dfs walk", "colour_ok", "to_string", "peq build", "sweep", "walk",
            "path records", "path qual", "select", "amb collect", "fixAmbiguity", "assemble", "trim", "revcomp", "consensus", "emit",
            "idle at round end", "colours: universe", "colours: rows", 0};
        static_assert(RL_NPROF == RTK_CNT_LANE_PROF2 - RTK_CNT_LANE_PROF, "counter map: the lane profile has RL_NPROF slots");
        const unsigned long long* p1 = cnt + RTK_CNT_LANE_PROF; const unsigned long long* p2 = cnt + RTK_CNT_LANE_PROF2;
        unsigned long long tot = 0; for (int i = 0; i < RL_NPROF; ++i) tot += p1[i];
        fprintf(stderr, "[rtk trace] k_regions_lanes lap profile (%.3g lane cycles):", double(tot));
        for (int i = 0; i < RL_NPROF; ++i) if (p1[i] && ln[i]) fprintf(stderr, " [%s %.4f]", ln[i], double(p1[i]) / double(tot ? tot : 1));
        fprintf(stderr, "\n");
        unsigned long long tw = 0; for (int i = 0; i < RL_NPROF; ++i) tw += p2[i];
        fprintf(stderr, "[rtk trace] k_regions_lanes wave-time estimate by slot (share of %.3g, lanes together):", double(tw) / 64.0);
        for (int i = 0; i < RL_NPROF; ++i)
            if (p2[i] && ln[i]) fprintf(stderr, " [%s %.4f x%.1f]", ln[i], double(p2[i]) / double(tw ? tw : 1), 64.0 * double(p1[i]) / double(p2[i]));
        fprintf(stderr, "\n");
    }
#endif
    fprintf(stderr, "[rtk trace] k_regions shares of %.3g wave cycles: colour %.3f paths %.3f consensus %.3f myers %.3f sets %.3f tostring %.3f pathqual %.3f "
                    "walk %.3f\n",
            double(cnt[RTK_CNT_CYC_TOTAL]), share(RTK_CNT_CYC_COLOUR), share(RTK_CNT_CYC_PATHS), share(RTK_CNT_CYC_CONSENSUS), share(RTK_CNT_CYC_MYERS),
            share(RTK_CNT_CYC_SETS),
            share(RTK_CNT_CYC_TOSTRING), share(RTK_CNT_CYC_PATHQUAL), share(RTK_CNT_WALK_CYCLES));
    fprintf(stderr, "[rtk trace] k_regions cycle shares: DFS bookkeeping %.3f (of which colour checks %.3f)\n", share(RTK_CNT_CYC_DFS), share(RTK_CNT_CYC_COLOUR_OK));
    fprintf(stderr, "[rtk trace] trims: by column %llu (of which stored %llu), by the distance call %llu, cycles %.3g; consensus calls: forward alignment resumed %llu, swept %llu\n",
            cnt[RTK_CNT_ROUTES + 0] + cnt[RTK_CNT_ROUTES + 1], cnt[RTK_CNT_ROUTES + 0], cnt[RTK_CNT_ROUTES + 2], double(cnt[RTK_CNT_FINE + RTK_FINE_TRIM]), cnt[RTK_CNT_ROUTES + 3], cnt[RTK_CNT_ROUTES + 4]);
    fprintf(stderr, "[rtk trace] fixAmbiguity linked-allele searches: run %llu, skipped %llu, entries produced %llu, cycles %.3g\n", cnt[RTK_CNT_FA_LINKED + 0], cnt[RTK_CNT_FA_LINKED + 1],
            cnt[RTK_CNT_FA_LINKED + 2], double(cnt[RTK_CNT_FINE + RTK_FINE_FA_LINKED]));
    fprintf(stderr, "[rtk trace] second strand of gap regions: run %llu, skipped %llu (the forward result decides), audit mismatches %llu\n", cnt[RTK_CNT_STRAND2 + 0], cnt[RTK_CNT_STRAND2 + 1], cnt[RTK_CNT_STRAND2 + 2]);
    fprintf(stderr, "[rtk trace] stored sweeps of the forward trims: walked for a consensus %llu (from a second sweep %llu), never walked %llu\n", cnt[RTK_CNT_PARK + 0], cnt[RTK_CNT_PARK_RESWEEPS], cnt[RTK_CNT_PARK + 1]);
    fprintf(stderr, "[rtk trace] colour selections answered by: small %llu, wide %llu, bits %llu, general %llu; audit mismatches %llu; handed on by the register program for room %llu\n", cnt[RTK_CNT_COLOURS + 0], cnt[RTK_CNT_COLOURS + 1], cnt[RTK_CNT_COLOURS + 2],
            cnt[RTK_CNT_COLOURS + 3], cnt[RTK_CNT_COLOURS + 4], cnt[RTK_CNT_COLOURS + 5]);
    fprintf(stderr, "[rtk trace] walks %llu moves %llu reloads %llu scalar steps %llu cycles %.3g tail cycles %.3g\n", cnt[RTK_CNT_WALK_CALLS], cnt[RTK_CNT_WALK_MOVES],
            cnt[RTK_CNT_WALK_RELOADS], cnt[RTK_CNT_WALK_SCALAR], double(cnt[RTK_CNT_WALK_CYCLES]), double(cnt[RTK_CNT_WALK_TAIL]));
}

// the stage's part of rtk_stats, from the timers and the copied counter block
static void region_stats(RegionRun& R, const unsigned long long* cnt) {
    rtk_batch* b = R.b; rtk_stats& st = b->stats;
    st.cyc_colour = cnt[RTK_CNT_CYC_COLOUR]; st.cyc_paths = cnt[RTK_CNT_CYC_PATHS]; st.cyc_consensus = cnt[RTK_CNT_CYC_CONSENSUS]; st.cyc_total = cnt[RTK_CNT_CYC_TOTAL];
    st.cyc_myers = cnt[RTK_CNT_CYC_MYERS]; st.cyc_sets = cnt[RTK_CNT_CYC_SETS]; st.cyc_tostring = cnt[RTK_CNT_CYC_TOSTRING]; st.cyc_pathqual = cnt[RTK_CNT_CYC_PATHQUAL];
    st.cyc_walk = cnt[RTK_CNT_WALK_CYCLES]; st.n_moves = cnt[RTK_CNT_WALK_MOVES];
    st.n_slots_exact = cnt[RTK_CNT_SLOTS_EXACT]; st.n_slots_inexact = cnt[RTK_CNT_SLOTS_INEXACT];
    st.ms_regions = R.t_enum.elapsed() + (R.n_regions ? R.t_easy.elapsed() : 0.0); // (enumeration + the regions without a graph walk)
    st.ms_lanes = R.lanes_on ? R.t_lanes.elapsed() : 0.0;
    st.ms_correct = R.ms_reg + ((R.lanes_on && !R.lanes_beside) ? st.ms_lanes : 0.0); // (beside: the span of the wave kernel's two launches contains the lane kernel)
    st.n_lane_handed = cnt[RTK_CNT_LANE_HANDED]; st.n_lane_regions = cnt[RTK_CNT_LANE_HANDED] + cnt[RTK_CNT_LANE_DONE];
    st.n_trim_stored = cnt[RTK_CNT_ROUTES + 0]; st.n_trim_column = cnt[RTK_CNT_ROUTES + 1]; st.n_trim_fallback = cnt[RTK_CNT_ROUTES + 2];
    st.n_consensus_resumed = cnt[RTK_CNT_ROUTES + 3]; st.n_consensus_swept = cnt[RTK_CNT_ROUTES + 4];
    st.n_fa_linked_run = cnt[RTK_CNT_FA_LINKED + 0]; st.n_fa_linked_skipped = cnt[RTK_CNT_FA_LINKED + 1]; st.n_fa_linked_entries = cnt[RTK_CNT_FA_LINKED + 2];
    st.n_strand2_run = cnt[RTK_CNT_STRAND2 + 0]; st.n_strand2_skipped = cnt[RTK_CNT_STRAND2 + 1]; st.n_strand2_audit_mismatch = cnt[RTK_CNT_STRAND2 + 2];
    st.n_park_walked = cnt[RTK_CNT_PARK + 0]; st.n_park_deferred = cnt[RTK_CNT_PARK + 1]; st.n_park_resweeps = cnt[RTK_CNT_PARK_RESWEEPS];
    st.n_colours_small = cnt[RTK_CNT_COLOURS + 0]; st.n_colours_wide = cnt[RTK_CNT_COLOURS + 1]; st.n_colours_bits = cnt[RTK_CNT_COLOURS + 2]; st.n_colours_general = cnt[RTK_CNT_COLOURS + 3];
    st.n_colours_audit_mismatch = cnt[RTK_CNT_COLOURS + 4]; st.n_colours_declined_fit = cnt[RTK_CNT_COLOURS + 5];
    st.ms_stitch = R.t_st.elapsed(); st.ms_total = b->t_all.elapsed();
    st.n_windows = b->n_bases;
    st.n_probes_exact = cnt[RTK_CNT_PROBES_EXACT]; st.n_probes_inexact = cnt[RTK_CNT_PROBES_INEXACT]; st.n_hits_inexact = cnt[RTK_CNT_HITS_INEXACT];
    st.n_regions = R.n_regions; st.n_region_items = R.n_regions; st.n_arena_overflow = R.n_ovf_total;
    st.n_expand = cnt[RTK_CNT_EXPAND]; st.n_colour_elem = cnt[RTK_CNT_COLOUR]; st.n_path_base = cnt[RTK_CNT_PATHBASE];
    st.n_align = cnt[RTK_CNT_ALIGN]; st.n_align_cells = cnt[RTK_CNT_CELLS];
    st.in_bases = b->n_bases; st.out_bases = R.out_top / 2;
}

// stage B: regions of every read (enumerate, correct, stitch) on the batch's stream; needs stage A of the same batch
extern "C" int rtk_batch_run_regions(rtk_batch* b, const rtk_opts* opts) {
    int rc = batch_precheck(b, opts, "rtk_batch_run_regions");
    if (rc) return rc;
    if (!b->seeded) return rtk_fail(RTK_ERR_ARG, "rtk_batch_run_regions: rtk_batch_run_seeds has not completed for this batch");
    if (opts->long_read_correct && !b->bv.qual.get())
        return rtk_fail(RTK_ERR_ARG, "rtk_batch_run_regions: the second pass (long_read_correct) needs a batch created with quality strings");
    rtk_graph* g = b->g;
    try {
        rtk_set_device(g->device);
        RegionRun R = {};
        R.b = b; R.g = g; R.ov = opts_view(opts); R.sm = b->stream; R.own_slab = opts->long_read_correct != 0;
        R.hold.g = g; R.hold.what = -1; R.slab.g = g;
        R.trace = rtk_knob_trace(); R.w0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < b->n; ++i) R.max_len = std::max<uint32_t>(R.max_len, static_cast<uint32_t>(b->roff[i + 1] - b->roff[i]));
        R.grid = default_grid();
        region_alloc(R);
        region_lane_class(R);
        R.lap("alloc");
        region_enumerate(R);
        R.lap("enum");
        region_easy(R);
        region_lanes(R);
        region_take_areas(R);
        rc = region_attempts(R);
        if (rc) return rc;
        R.hold.release();
        R.lap("regions");
        rc = region_stitch(R);
        if (rc) return rc;
        unsigned long long cnt[RTK_CNT_TOTAL]; rtk_d2h_s(cnt, b->bv.counters, sizeof(cnt), R.sm);
        if (R.trace) region_trace_report(cnt);
        region_stats(R, cnt);
        R.lap("done");
        if (b->h_out) { g->stage_give(b->h_out, b->h_out_bytes); b->h_out = nullptr; } // a re-run invalidates the fetched view
        b->ran = true; b->seeded = false;
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return RTK_OK;
}

extern "C" int rtk_batch_run(rtk_batch* b, const rtk_opts* opts) {
    const int rc = rtk_batch_run_seeds(b, opts);
    return rc ? rc : rtk_batch_run_regions(b, opts);
}

// D2H of the packed records into pinned staging memory owned by the batch (once; repeated calls return the same view)
static int batch_fetch_host(rtk_batch* b) {
    if (b->h_out) return RTK_OK;
    rtk_set_device(b->g->device);
    const auto tf0 = std::chrono::steady_clock::now();
    unsigned long long out_top = 0; rtk_d2h_s(&out_top, b->rb.out_top, 8, b->stream);
    const auto tf1 = std::chrono::steady_clock::now();
    b->h_out = b->g->stage_take(out_top + 8, &b->h_out_bytes);
    const auto tf2 = std::chrono::steady_clock::now();
    b->h_off.resize(b->n); b->h_sl.resize(b->n); b->h_ql.resize(b->n);
    if (out_top) rtk_check_async_d2h(b->h_out, b->rb.out_pool, out_top, b->stream);
    rtk_d2h_s(b->h_off.data(), b->rb.out_off, 8ull * b->n, b->stream); rtk_d2h_s(b->h_sl.data(), b->rb.out_seq_len, 4ull * b->n, b->stream); rtk_d2h_s(b->h_ql.data(), b->rb.out_qual_len, 4ull * b->n, b->stream);
    if (rtk_knob_trace()) { auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b_) { return std::chrono::duration<double, std::milli>(b_ - a).count(); }; fprintf(stderr, "[rtk trace] fetch: wait for the stream %.2f ms, staging buffer %.2f ms, %.1f MB to the host %.2f ms\n", ms(tf0, tf1), ms(tf1, tf2), out_top / 1048576.0, ms(tf2, std::chrono::steady_clock::now())); }
    for (uint32_t i = 0; i < b->n; ++i) {
        const char* bad = nullptr;
        if (b->h_sl[i] != b->h_ql[i]) bad = "rtk_batch_fetch: sequence and quality lengths differ for a read";
        else if (b->h_off[i] + 2ull * b->h_sl[i] > out_top) bad = "rtk_batch_fetch: record outside the output pool";
        if (bad) { rtk_ssync(b->stream); b->g->stage_give(b->h_out, b->h_out_bytes); b->h_out = nullptr; return rtk_fail(RTK_ERR_DEVICE, bad); } // a rejected view is never handed out by a later call
    }
    return RTK_OK;
}

extern "C" int rtk_batch_fetch_view(rtk_batch* b, const char** pool, const uint64_t** off, const uint32_t** len) {
    if (!b || !pool || !off || !len) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch_view: null argument");
    if (!b->ran) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch_view: rtk_batch_run has not completed");
    try { const int rc = batch_fetch_host(b); if (rc) return rc; }
    catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    *pool = static_cast<const char*>(b->h_out); *off = b->h_off.data(); *len = b->h_sl.data();
    return RTK_OK;
}

extern "C" int rtk_batch_fetch(rtk_batch* b, char** out_seq, char** out_qual, uint32_t* out_len) {
    if (!b || !out_seq || !out_qual || !out_len) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch: null argument");
    if (!b->ran) return rtk_fail(RTK_ERR_ARG, "rtk_batch_fetch: rtk_batch_run has not completed");
    try {
        const int rc = batch_fetch_host(b); if (rc) return rc; // every length is validated before anything is allocated
        const char* pool = static_cast<const char*>(b->h_out);
        for (uint32_t i = 0; i < b->n; ++i) { out_seq[i] = nullptr; out_qual[i] = nullptr; }
        // the caller's strings: two allocations and two copies per read, on up to four threads for a big ticket (like the packing of rtk_batch_create; one thread moves
        // ~2 GB/s into fresh allocations, a 64 Mb ticket is 128 MB of records)
        std::atomic<bool> oom(false);
        auto copy_range = [&](uint32_t lo, uint32_t hi) {
            for (uint32_t i = lo; i < hi && !oom.load(std::memory_order_relaxed); ++i) {
                const uint32_t sl = b->h_sl[i];
                out_seq[i] = static_cast<char*>(malloc(sl + 1)); out_qual[i] = static_cast<char*>(malloc(sl + 1));
                if (!out_seq[i] || !out_qual[i]) { oom.store(true); return; }
                memcpy(out_seq[i], pool + b->h_off[i], sl); out_seq[i][sl] = 0;
                memcpy(out_qual[i], pool + b->h_off[i] + sl, sl); out_qual[i][sl] = 0;
                out_len[i] = sl;
            }
        };
        {
            const uint32_t n_thr = (b->n_bases >= (4u << 20) && b->n >= 8) ? 4u : 1u;
            std::vector<uint32_t> cut(n_thr + 1, b->n); cut[0] = 0;
            for (uint32_t t = 1, i = 0; t < n_thr; ++t) { const uint64_t want = b->n_bases / n_thr * t; while (i < b->n && b->roff[i] < want) ++i; cut[t] = i; }
            std::vector<std::thread> thr;
            for (uint32_t t = 1; t < n_thr; ++t) thr.emplace_back(copy_range, cut[t], cut[t + 1]);
            copy_range(cut[0], cut[1]);
            for (size_t t = 0; t < thr.size(); ++t) thr[t].join();
        }
        if (oom.load()) { for (uint32_t j = 0; j < b->n; ++j) { free(out_seq[j]); free(out_qual[j]); out_seq[j] = nullptr; out_qual[j] = nullptr; } return rtk_fail(RTK_ERR_DEVICE, "rtk_batch_fetch: out of host memory"); }
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, e.what()); }
    return RTK_OK;
}

extern "C" int rtk_batch_get_stats(const rtk_batch* b, rtk_stats* stats) { if (!b || !stats) return rtk_fail(RTK_ERR_ARG, "rtk_batch_get_stats: null"); *stats = b->stats; return RTK_OK; }

// ------------------------------------------------------------------------------------------------ ticket coalescing (rtk_correct_batch)
// The reference's workers each take a ticket of >= 1 MiB of bases (src/Common.hpp:138, src/Ratatosk.cpp:757-772) and call the per-read loop on it; a launch
// of a ticket that small lasts as long as its longest read and its slowest region with most of the device idle (2 x 10^8 bases/s whatever the number of
// callers). So tickets of concurrent callers are merged: a caller that arrives while a group is being gathered joins it, the group runs as ONE batch
// (one pack + H2D, one set of launches, one D2H), every caller copies its own reads out of the group's pinned view. Who gathers: the first caller whose
// ticket is still waiting when nobody else gathers. How long it gathers: until the group holds RTK_COALESCE_BASES (16 Mi) bases, else
//  * RTK_COALESCE_WAIT_US (1 500) from its own arrival in every case -- except when it is alone (nothing queued, nothing in flight, the last group was a
//    single ticket): then not at all;
//  * groups in flight: beyond that until the youngest of them HAS the work areas of its region stage (the region stage is 85 % of a launch; two small groups run it side by
//    side on one half of the graph's work areas each, rtk_graph::region_slab_take; the seed stage, pack and H2D of the next group run beside them, and whoever
//    arrives until then joins for free), with at most three in flight. Merged: first-pass tickets below the
// byte cap with the same options and the same kind of input (with / without qualities). Results are those of the tickets run one by one: reads are
// independent units (SURVEY.md 8(e)); tests/test_coalesce.py holds that ticket by ticket against the oracle.
struct CoGroup { rtk_batch* b = nullptr; const char* pool = nullptr; const uint64_t* off = nullptr; const uint32_t* len = nullptr; std::atomic<int> left{0}; };
struct CoTicket {
    const rtk_opts* opts; uint32_t n; const char* const* seq; const char* const* qual; const uint32_t* len; uint64_t bases;
    bool taken = false, done = false, alone_after_all = false; int rc = 0; std::string err; CoGroup* grp = nullptr; uint32_t first = 0;
};
static bool co_compatible(const CoTicket& a, const CoTicket& b) { return (a.qual == nullptr) == (b.qual == nullptr) && memcmp(a.opts, b.opts, sizeof(rtk_opts)) == 0; }

extern "C" int rtk_coalesce_stats(rtk_graph* g, uint64_t* n_groups, uint64_t* n_tickets) {
    if (!g || !n_groups || !n_tickets) return rtk_fail(RTK_ERR_ARG, "rtk_coalesce_stats: null argument");
    std::lock_guard<std::mutex> lk(g->co_m); *n_groups = g->co_groups; *n_tickets = g->co_tickets; return RTK_OK;
}

// one call on its own: the batch of one ticket
static int correct_batch_alone(rtk_graph* g, const rtk_opts* opts, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len, char** out_seq, char** out_qual, uint32_t* out_len) {
    rtk_batch* b = nullptr;
    const bool trace = rtk_knob_trace();
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    int rc = rtk_batch_create(g, n, seq, qual, len, &b);
    if (rc) return rc;
    const double t_create = ms(t0); const auto t1 = std::chrono::steady_clock::now();
    rc = rtk_batch_run(b, opts);
    const double t_run = ms(t1); const auto t2 = std::chrono::steady_clock::now();
    if (rc == RTK_OK) rc = rtk_batch_fetch(b, out_seq, out_qual, out_len);
    const double t_fetch = ms(t2); const auto t3 = std::chrono::steady_clock::now();
    rtk_batch_free(b);
    if (trace) fprintf(stderr, "[rtk trace] correct_batch: create %.1f ms, run %.1f ms, fetch %.1f ms, free %.1f ms\n", t_create, t_run, t_fetch, ms(t3));
    return rc;
}

extern "C" int rtk_correct_batch(rtk_graph* g, const rtk_opts* opts, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len,
                                 char** out_seq, char** out_qual, uint32_t* out_len) {
    if (!g || !opts || (n && (!seq || !len || !out_seq || !out_qual || !out_len))) return rtk_fail(RTK_ERR_ARG, "rtk_correct_batch: null argument");
    if (!opts_ok(opts)) return rtk_fail(RTK_ERR_ARG, "rtk_correct_batch: rtk_opts was not filled by this library's rtk_opts_default (struct_size does not match: older header, or a zero-filled struct)");
    if (!g->on_device) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_correct_batch: graph is not resident on a device (call rtk_graph_upload); there is no CPU fallback");
    if (n == 0) return RTK_OK;
    uint64_t bases = 0; for (uint32_t i = 0; i < n; ++i) bases += len[i];
    const uint64_t cap = rtk_knob_coalesce_bases();
    if (cap == 0 || bases >= cap || opts->long_read_correct) return correct_batch_alone(g, opts, n, seq, qual, len, out_seq, out_qual, out_len);

    CoTicket me; me.opts = opts; me.n = n; me.seq = seq; me.qual = qual; me.len = len; me.bases = bases;
    std::unique_lock<std::mutex> lk(g->co_m);
    g->co_q.push_back(&me);
    g->co_cv.notify_all(); // (a gathering caller counts again)
    while (!me.done) {
        if (me.taken || g->co_gathering) { g->co_cv.wait(lk); continue; }
        // ---- this caller gathers a group around its own ticket
        g->co_gathering = true;
        const bool alone = g->co_q.size() == 1 && g->co_running == 0 && g->co_last_group <= 1;
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(alone ? 0L : rtk_knob_coalesce_wait_us());
        const bool cold = g->co_running == 0;
        while (true) {
            uint64_t sum = 0; for (size_t i = 0; i < g->co_q.size(); ++i) if (co_compatible(*g->co_q[i], me)) sum += g->co_q[i]->bases;
            if (sum >= cap) break;
            const bool late = std::chrono::steady_clock::now() >= deadline;
            // the bounded wait holds in every case (the callers of a group that has just finished come back within a millisecond or two of each other: launching for
            // the first of them would split them into many small groups); beyond it, as long as a younger group has not got its work areas or three are in flight
            if (late && (g->co_running == 0 || (g->co_pre_region == 0 && g->co_running < 3))) break;
            if (late) g->co_cv.wait(lk); else g->co_cv.wait_until(lk, deadline); // (late: woken by an arrival, by a group's stage change, by a group that finished)
        }
        // A group takes at most half of the tickets that are around (waiting here + travelling in the groups in flight), when there are four or more: two groups then
        // alternate -- the host side of one (pack, H2D, D2H, the callers' copies and their way back with the next ticket) beside the kernels of the other -- instead
        // of everybody travelling in one group whose stages nothing overlaps (traced: 15 of 16 callers in one group, 37 ms per 16 Mb, profiles/r06_coalesce_trace.txt).
        uint64_t take_cap = cap; uint32_t take_n = 0xFFFFFFFFu;
        { uint32_t nw = 0; for (size_t i = 0; i < g->co_q.size(); ++i) if (co_compatible(*g->co_q[i], me)) ++nw;
          const uint32_t split = rtk_knob_coalesce_split();
          const uint32_t around = nw + g->co_inflight_tickets; if (around >= 2 * split) take_n = (around + split - 1) / split; }
        (void)cold;
        std::vector<CoTicket*> grp; uint64_t sum = 0;
        for (size_t i = 0; i < g->co_q.size();) {
            CoTicket* t = g->co_q[i];
            if (((sum < take_cap && grp.size() < take_n) || t == &me) && co_compatible(*t, me)) { t->taken = true; sum += t->bases; grp.push_back(t); g->co_q.erase(g->co_q.begin() + static_cast<long>(i)); } else ++i;
        }
        g->co_gathering = false; g->co_running += 1; g->co_pre_region += 1; g->co_last_group = static_cast<uint32_t>(grp.size()); g->co_inflight_tickets += static_cast<uint32_t>(grp.size()); g->co_groups += 1; g->co_tickets += grp.size();
        g->co_cv.notify_all(); // a ticket left behind (other options) finds a gatherer in its own caller
        lk.unlock();
        // ---- the group as one batch
        int rc = RTK_OK; std::string err; CoGroup* cg = new CoGroup();
        struct Pace { rtk_graph* g; bool in_regions; } pace = {g, false};
        auto enter_regions_fn = [](void* p_) { Pace* p = static_cast<Pace*>(p_); if (!p->in_regions) { p->in_regions = true; std::lock_guard<std::mutex> l2(p->g->co_m); p->g->co_pre_region -= 1; p->g->co_cv.notify_all(); } };
        auto enter_regions = [&]() { enter_regions_fn(&pace); };
        if (grp.size() == 1) { // nobody joined: the plain path, outputs straight into the caller's arrays
            delete cg; cg = nullptr;
            rtk_batch* b1 = nullptr;
            rc = rtk_batch_create(g, n, seq, qual, len, &b1);
            if (rc == RTK_OK) { b1->on_region_slab = enter_regions_fn; b1->on_region_slab_arg = &pace; rc = rtk_batch_run_seeds(b1, opts); }
            if (rc == RTK_OK) rc = rtk_batch_run_regions(b1, opts);
            enter_regions();
            if (rc == RTK_OK) rc = rtk_batch_fetch(b1, out_seq, out_qual, out_len);
            if (rc) err = rtk_last_error();
            if (b1) rtk_batch_free(b1);
        } else {
            uint32_t tot = 0; for (size_t i = 0; i < grp.size(); ++i) { grp[i]->first = tot; tot += grp[i]->n; }
            std::vector<const char*> sa(tot), qa(qual ? tot : 0); std::vector<uint32_t> la(tot);
            for (size_t i = 0; i < grp.size(); ++i) for (uint32_t j = 0; j < grp[i]->n; ++j) { sa[grp[i]->first + j] = grp[i]->seq[j]; la[grp[i]->first + j] = grp[i]->len[j]; if (qual) qa[grp[i]->first + j] = grp[i]->qual[j]; }
            const bool tr_ = rtk_knob_trace(); static const auto t_epoch = std::chrono::steady_clock::now();
            auto now_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_epoch).count(); };
            const double tq0 = now_ms();
            rc = rtk_batch_create(g, tot, sa.data(), qual ? qa.data() : nullptr, la.data(), &cg->b);
            const double tq1 = now_ms();
            if (rc == RTK_OK) { cg->b->on_region_slab = enter_regions_fn; cg->b->on_region_slab_arg = &pace; rc = rtk_batch_run_seeds(cg->b, opts); }
            const double tq2 = now_ms();
            if (rc == RTK_OK) rc = rtk_batch_run_regions(cg->b, opts);
            enter_regions();
            const double tq3 = now_ms();
            if (rc == RTK_OK) rc = rtk_batch_fetch_view(cg->b, &cg->pool, &cg->off, &cg->len);
            if (tr_) fprintf(stderr, "[rtk trace] correct_batch group at %.1f ms: %zu tickets, %u reads, %.2f Mb; create %.2f seeds %.2f (kernels %.2f) regions %.2f (k_regions %.2f) fetch %.2f ms (rc %d)\n", tq0, grp.size(), tot, sum / 1e6, tq1 - tq0, tq2 - tq1,
                            cg->b ? cg->b->stats.ms_lookup_exact + cg->b->stats.ms_mask + cg->b->stats.ms_lookup_inexact + cg->b->stats.ms_seeds : 0.0, tq3 - tq2, cg->b ? cg->b->stats.ms_correct : 0.0, now_ms() - tq3, rc);
            if (rc == RTK_OK && rtk_knob_test_coalesce_fail()) rc = rtk_fail(RTK_ERR_DEVICE, "test hook: the merged batch is reported as failed"); // (tests/test_coalesce.py: the members must come through on their own)
            if (rc) { err = rtk_last_error(); if (cg->b) rtk_batch_free(cg->b); delete cg; cg = nullptr; }
            else cg->left.store(static_cast<int>(grp.size()));
        }
        enter_regions();
        lk.lock();
        g->co_running -= 1; g->co_inflight_tickets -= static_cast<uint32_t>(grp.size());
        // a group that failed (a capacity of the merged batch, a bad ticket among them) does not fail its members: every one of them runs its own ticket again, alone
        const bool redo = rc != RTK_OK && grp.size() > 1;
        for (size_t i = 0; i < grp.size(); ++i) { grp[i]->rc = redo ? RTK_OK : rc; grp[i]->err = err; grp[i]->grp = cg; grp[i]->alone_after_all = redo; grp[i]->done = true; }
        g->co_cv.notify_all();
    }
    lk.unlock();
    if (me.rc) return rtk_fail(me.rc, me.err);
    if (me.alone_after_all) return correct_batch_alone(g, opts, n, seq, qual, len, out_seq, out_qual, out_len);
    if (!me.grp) return RTK_OK; // ran on its own: outputs are in place
    // ---- this caller's reads out of the group's pinned view (every caller copies its own, side by side); the last one releases the batch
    CoGroup* cg = me.grp; int rc = RTK_OK;
    for (uint32_t i = 0; i < n; ++i) { out_seq[i] = nullptr; out_qual[i] = nullptr; }
    for (uint32_t i = 0; i < n && rc == RTK_OK; ++i) {
        const uint32_t r = me.first + i, sl = cg->len[r];
        out_seq[i] = static_cast<char*>(malloc(sl + 1)); out_qual[i] = static_cast<char*>(malloc(sl + 1));
        if (!out_seq[i] || !out_qual[i]) { for (uint32_t j = 0; j <= i; ++j) { free(out_seq[j]); free(out_qual[j]); out_seq[j] = nullptr; out_qual[j] = nullptr; } rc = rtk_fail(RTK_ERR_DEVICE, "rtk_correct_batch: out of host memory"); break; }
        memcpy(out_seq[i], cg->pool + cg->off[r], sl); out_seq[i][sl] = 0;
        memcpy(out_qual[i], cg->pool + cg->off[r] + sl, sl); out_qual[i][sl] = 0;
        out_len[i] = sl;
    }
    if (cg->left.fetch_sub(1) == 1) { rtk_batch_free(cg->b); delete cg; }
    return rc;
}

// Reserves the two per-wave scratch slabs a graph on `device` will need for reads up to max_read_len (sizes of the first attempt of the
// seed and region stages), so that their allocation overlaps whatever the caller does next (typically rtk_graph_load).
// Second pass: every ticket in flight owns two work areas (phasing step, region stage). n_tickets x the two sizes reserved ahead, like
// rtk_reserve_scratch does for the first pass; a ticket takes the smallest reserved slab that is large enough before it allocates.
extern "C" int rtk_reserve_second_pass(int device, uint32_t n_tickets, uint64_t phase_bytes, uint64_t region_bytes) {
#ifdef RTK_SIM
    (void)device; (void)n_tickets; (void)phase_bytes; (void)region_bytes; return RTK_OK; // the simulator's areas are small and allocated on demand
#endif
    try {
        rtk_set_device(device);
        { // once per device: the work areas of the per-read seed kernels (one slab per graph, shared by its tickets under a lock)
            static std::vector<int> seeded; bool first = false;
            { std::lock_guard<std::mutex> lk(g_reserved_lock); if (std::find(seeded.begin(), seeded.end(), device) == seeded.end()) { seeded.push_back(device); first = true; } }
            if (first) {
                SeedScratchCfg sc; sc.set_cap = 32768u; sc.v_cap = 32768u; sc.s_cap = 131072u + 64;
                ReservedSlab r; r.device = device; r.bytes = seed_scratch_bytes(sc) * static_cast<uint64_t>(seed_waves()); r.p = rtk_dmalloc(r.bytes);
                std::lock_guard<std::mutex> lk(g_reserved_lock); g_reserved.push_back(r);
            }
        }
        for (uint32_t t = 0; t < n_tickets; ++t) for (int i = 0; i < 2; ++i) {
            const uint64_t want = i == 0 ? phase_bytes : region_bytes;
            if (!want) continue;
            // never more than what is free now minus a margin for the graph image and the batches: a ticket whose areas are not reserved allocates them itself
#ifndef RTK_SIM
            size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) != hipSuccess) break;
            if (static_cast<uint64_t>(fr) < want + (static_cast<uint64_t>(tot) / 4)) return rtk_fail(RTK_ERR_DEVICE, "rtk_reserve_second_pass: not reserved (less than a quarter of the device memory would stay free)");
#endif
            ReservedSlab r; r.device = device; r.bytes = want; r.p = rtk_dmalloc(want);
            std::lock_guard<std::mutex> lk(g_reserved_lock); g_reserved.push_back(r);
        }
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_reserve_second_pass: ") + e.what()); }
    return RTK_OK;
}

extern "C" int rtk_reserve_scratch(int device, uint32_t max_read_len) {
    try {
        rtk_set_device(device);
        SeedScratchCfg sc; sc.set_cap = 32768u; sc.v_cap = 32768u; { uint32_t q = 131072u; while (q < max_read_len) q <<= 1; sc.s_cap = q + 64; }
#ifdef RTK_SIM
        const uint64_t n_seed_waves = 16, reg_waves = 16;
#else
        const uint64_t n_seed_waves = static_cast<uint64_t>(seed_waves()), reg_waves = static_cast<uint64_t>(rtk_knob_region_waves());
#endif
#ifdef RTK_SIM
        uint64_t reg_bytes = region_scratch_bytes(region_cfg(max_read_len, 0)) * reg_waves;
#else
        (void)reg_waves;
        uint64_t reg_bytes = region_scratch_bytes(region_cfg(max_read_len, 0)) * static_cast<uint64_t>(region_waves_that_fit(region_scratch_bytes(region_cfg(max_read_len, 0)), 0, rtk_knob_trace()));
#endif
#ifndef RTK_SIM
        if (region_compact()) reg_bytes = std::max<uint64_t>(reg_bytes, region_scratch_bytes(region_cfg(max_read_len, 1)) * 1024ull); // the full-size areas of the redo launch share the slab
#endif
        const uint64_t want[2] = { seed_scratch_bytes(sc) * n_seed_waves, reg_bytes };
        for (int i = 0; i < 2; ++i) {
            ReservedSlab r; r.device = device; r.bytes = want[i]; r.p = rtk_dmalloc(want[i]);
            std::lock_guard<std::mutex> lk(g_reserved_lock);
            g_reserved.push_back(r);
        }
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_reserve_scratch: ") + e.what()); }
    return RTK_OK;
}
