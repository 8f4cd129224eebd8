// Anchor stage, what the two 1-edit searches (rtk_seed_enum.h, rtk_seed_seeded.h) share: the kinds of edit and the [A2] rule, which windows of a tile are
// searched and with which characters, and a wave's slice of the raw-hit pool.
#ifndef RTK_SEED_WINDOW_H
#define RTK_SEED_WINDOW_H

#include "rtk_acgt.h"
#include "rtk_seed_types.h"
#include "rtk_wave.h"

// kinds of 1-edit relation between a window and a graph k-mer ([A2] switch: rtk_opts::a2_exclusive)
#define RTK_EDIT_SUB 1u
#define RTK_EDIT_INS 2u
#define RTK_EDIT_DEL 4u
// [A2] exclusive readings: of the kinds of edit that matched a window (`any`), the one whose hits are kept. mode 1: substitution -> insertion -> deletion
// (the order of the blocks in Bifrost's searchSequence as we remember it); mode 2: insertion -> deletion -> substitution (the order of its parameters)
RTK_DEV uint32_t rtk_a2_keep(uint32_t any, uint32_t mode) {
    if (mode == 2u) return (any & RTK_EDIT_INS) ? RTK_EDIT_INS : ((any & RTK_EDIT_DEL) ? RTK_EDIT_DEL : (any & RTK_EDIT_SUB));
    return any & (0u - any);
}

struct RtkWinCode { uint64_t c_k1; uint32_t ck, ck1; bool cand; }; // a window: its first k - 1 characters, the next two (4 = unusable), is it searched at all

// window_code(bb, have_S, S, n_ok) -> the window at base position bb of a tile whose first base belongs to read lo_tile (rtk_owner_read). Whether it may be searched is
// the window's own matter: its read, the characters that read still has (rend), the leading A/C/G/T of the masked copy `text` (n_ok). S = its k + 1 characters as a code
// when the caller has them (bit planes), else they are packed from text here. The closure holds references to the tile program's own variables, which must outlive it.
// (A closure and not a plain function of ten arguments: k_inexact's code is the same to the instruction with this form alone.)
RTK_DEV auto rtk_window_coder(const BatchView& bv, const uint64_t* const& roff, const uint32_t& n_reads, const uint32_t& lo_tile, const unsigned char* const& text, const int& k) {
    return [&](uint64_t bb, bool have_S, uint64_t S, int n_ok) {
        RtkWinCode w; w.cand = false; w.c_k1 = 0; w.ck = 4; w.ck1 = 4;
        if (bb < bv.n_bases) {
            uint32_t lo = lo_tile; // owning read: steps forward from the read of the tile's first base
            while (lo + 1 < n_reads && roff[lo + 1] <= bb) ++lo;
            const uint64_t rend = roff[lo + 1];
            if (bb + static_cast<uint64_t>(k) <= rend && rend - roff[lo] > static_cast<uint64_t>(k)) {
                if (!have_S) S = rtk_pack_acgt(text + bb, k + 1, &n_ok); // k + 1 characters packed without per-character branches (the masked copy is padded by 64 bytes)
                if (n_ok >= k - 1) {
                    w.cand = true; w.c_k1 = S >> 4;
                    if (n_ok >= k) { w.ck = static_cast<uint32_t>((S >> 2) & 3ull); if (n_ok >= k + 1 && bb + static_cast<uint64_t>(k) + 1 <= rend) w.ck1 = static_cast<uint32_t>(S & 3ull); }
                }
            }
        }
        return w;
    };
}

// the same window for a caller that asks once per tile
RTK_DEV RtkWinCode rtk_window_code(const BatchView& bv, const uint64_t* roff, uint32_t n_reads, uint32_t lo_tile, const unsigned char* text, int k, uint64_t bb) {
    return rtk_window_coder(bv, roff, n_reads, lo_tile, text, k)(bb, false, 0, 0);
}

// `total` (> 0, wave-uniform) entries of the raw-hit pool from the wave's private slice -> the index of the first. A slice that holds fewer is replaced by a new one
// (one device atomic per RTK_POOL_CHUNK entries; the tail of the old slice is abandoned). The caller holds the index against BatchView::ipool_cap before it writes.
RTK_DEV unsigned long long rtk_pool_take(const BatchView& bv, PoolChunk* chunk, int total) {
    if (chunk->left < static_cast<uint32_t>(total)) {
        unsigned long long nb = 0;
        if (rtk_lane() == 0) nb = rtk_atomic_add(bv.ipool_top, static_cast<unsigned long long>(RTK_POOL_CHUNK));
        chunk->base = rtk_shfl(nb, 0); chunk->left = RTK_POOL_CHUNK;
    }
    const unsigned long long pbase = chunk->base;
    chunk->base += static_cast<unsigned long long>(total); chunk->left -= static_cast<uint32_t>(total);
    return pbase;
}

#endif
