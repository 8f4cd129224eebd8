// Region stage, ResultCorrection (reference: src/ResultCorrection.hpp: the Roaring set of corrected old positions as a word-wise bitmap,
// getLengthCorrectedRegion :117-128, getLengthUncorrectedRegion :130-142, reverseComplement :72-88) and the appenders of the growing
// corrected strings.
#ifndef RTK_REGION_RESULT_H
#define RTK_REGION_RESULT_H

#include "rtk_region_paths.h"

// ------------------------------------------------------------------------------------------------ ResultCorrection (src/ResultCorrection.hpp)

// position bitmaps (ResultCorrection's Roaring set of corrected old positions): word-wise, one word per lane
RTK_DEV void rtk_bm_add_range(uint64_t* bm, uint32_t a, uint32_t b) { // [a, b)
    if (b <= a) return;
    const uint32_t w0 = a >> 6, w1 = (b - 1) >> 6;
    for (uint32_t w = w0 + static_cast<uint32_t>(rtk_lane()); w <= w1; w += RTK_WAVE) {
        const uint32_t lo = (w == w0) ? (a & 63u) : 0u, hi = (w == w1) ? ((b - 1) & 63u) : 63u;
        const uint64_t mask = ((hi == 63u) ? ~0ull : ((1ull << (hi + 1)) - 1ull)) & ~((1ull << lo) - 1ull);
        bm[w] |= mask;
    }
    rtk_sync();
}
RTK_DEV uint32_t rtk_bm_card(const uint64_t* bm, uint32_t n) {
    int c = 0;
    for (uint32_t w = static_cast<uint32_t>(rtk_lane()); w < (n + 63) / 64; w += RTK_WAVE) c += rtk_popc(bm[w]);
    return static_cast<uint32_t>(rtk_u(rtk_wave_sum(c)));
}
RTK_DEV bool rtk_bm_get(const uint64_t* bm, uint32_t i) { return (bm[i >> 6] >> (i & 63)) & 1ull; }
// first position >= p (capped at n) whose bit equals `want`
RTK_DEV uint32_t rtk_bm_next(const uint64_t* bm, uint32_t n, uint32_t p, bool want) {
    if (p >= n) return n;
    const uint32_t words = (n + 63) / 64;
    for (uint32_t w0 = p >> 6; w0 < words; w0 += RTK_WAVE) {
        const uint32_t w = w0 + static_cast<uint32_t>(rtk_lane());
        uint64_t x = 0;
        if (w < words) { x = want ? bm[w] : ~bm[w]; if (w == (p >> 6)) x &= ~((1ull << (p & 63u)) - 1ull); }
        const uint64_t bal = rtk_ballot(x != 0);
        if (bal) {
            const int l = rtk_ffs(bal) - 1;
            const uint32_t pos = 64u * (w0 + static_cast<uint32_t>(l)) + static_cast<uint32_t>(rtk_ffs(rtk_shfl(x, l)) - 1);
            return rtk_u(pos < n ? pos : n);
        }
    }
    return n;
}
RTK_DEV uint32_t rtk_rc_len_corrected(const ResCorr& r, uint32_t p) { return rtk_bm_next(r.bm, r.old_len, p, false) - (p < r.old_len ? p : r.old_len); } // :117-128
RTK_DEV uint32_t rtk_rc_len_uncorrected(const ResCorr& r, uint32_t p) { return rtk_bm_next(r.bm, r.old_len, p, true) - (p < r.old_len ? p : r.old_len); } // :130-142
// 64 bits of the bitmap starting at bit `lo` (may be negative; bits outside the words read as 0)
RTK_DEV uint64_t rtk_bm_window(const uint64_t* bm, uint32_t words, int64_t lo) {
    if (lo <= -64) return 0ull;
    if (lo < 0) return words ? (bm[0] << static_cast<uint32_t>(-lo)) : 0ull;
    const uint32_t w = static_cast<uint32_t>(lo >> 6), sh = static_cast<uint32_t>(lo & 63);
    uint64_t x = 0;
    if (w < words) x = bm[w] >> sh;
    if (sh && w + 1 < words) x |= bm[w + 1] << (64u - sh);
    return x;
}

RTK_FN void rtk_rc_reverse_complement(RegionScratch& s_, ResCorr& r_, uint64_t* tmp_bm_, char* tmp_) {
    RegionScratch& s = *rtk_u(&s_); RTK_ASSUME_LDS(&s); ResCorr& r = *rtk_u(&r_); uint64_t* tmp_bm = rtk_u(tmp_bm_); char* tmp = rtk_u(tmp_); // :72-88
    if (r.seq_len == 0) return;
    const uint32_t words = (r.old_len + 63) / 64;
    // new bit j = old bit old_len-1-j: output word ow is the bit reversal of the 64 old bits ending at old_len-1-64*ow
    for (uint32_t ow = static_cast<uint32_t>(rtk_lane()); ow < words; ow += RTK_WAVE)
        tmp_bm[ow] = rtk_brev64(rtk_bm_window(r.bm, words, static_cast<int64_t>(r.old_len) - 1 - 64ll * ow - 63));
    rtk_sync();
    for (uint32_t w = static_cast<uint32_t>(rtk_lane()); w < words; w += RTK_WAVE) r.bm[w] = tmp_bm[w];
    rtk_sync();
    for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < r.seq_len; i += RTK_WAVE) tmp[i] = rtk_comp(r.seq[r.seq_len - 1 - i]);
    rtk_sync(); rtk_wcopy(r.seq, tmp, r.seq_len);
    for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < r.qual_len; i += RTK_WAVE) tmp[i] = r.qual[r.qual_len - 1 - i];
    rtk_sync(); rtk_wcopy(r.qual, tmp, r.qual_len);
    (void)s;
}

// appenders for the growing corrected strings
RTK_FN_LEAF void rtk_app(RegionScratch& s_, char* dst_, uint32_t* len_, const char* src_, uint32_t n_) {
    RegionScratch& s = *rtk_u(&s_); RTK_ASSUME_LDS(&s); char* dst = rtk_u(dst_); uint32_t* len = rtk_u(len_); const char* src = rtk_u(src_); uint32_t n = rtk_u(n_); if (*len + n > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return; } rtk_wcopy(dst + *len, src, n); *len += n; }
RTK_FN_LEAF void rtk_app_fill(RegionScratch& s_, char* dst_, uint32_t* len_, char ch_, uint32_t n_) {
    RegionScratch& s = *rtk_u(&s_); RTK_ASSUME_LDS(&s); char* dst = rtk_u(dst_); uint32_t* len = rtk_u(len_); char ch = rtk_u(ch_); uint32_t n = rtk_u(n_); if (*len + n > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return; } rtk_wfill(dst + *len, ch, n); *len += n; }

#endif
