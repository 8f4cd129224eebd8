// The Advance_Block step (Myers 1999 / Hyyro 2003) on 64- and 32-bit words, and the query profile it consumes: the table indexed by
// character class, a word of it for any target byte, and the four A/C/G/T words of one query word that the device sweeps keep in registers.
#ifndef RTK_MYERS_STEP_H
#define RTK_MYERS_STEP_H
#include "rtk_acgt.h"
#include "rtk_myers_types.h"

// One Advance_Block step (Myers 1999 / Hyyro 2003). hin, return value in {-1,0,1}; bit = row whose horizontal delta leaves the word.
RTK_DEV int rtk_myers_step(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, int bit, uint64_t& Ph_out, uint64_t& Mh_out) {
    const uint64_t pv = Pv, mv = Mv;
    const uint64_t Xv = Eq | mv;
    if (hin < 0) Eq |= 1ull;
    const uint64_t Xh = (((Eq & pv) + pv) ^ pv) | Eq;
    uint64_t Ph = mv | ~(Xh | pv);
    uint64_t Mh = pv & Xh;
    Ph_out = Ph; Mh_out = Mh;
    const int hout = static_cast<int>((Ph >> bit) & 1ull) - static_cast<int>((Mh >> bit) & 1ull);
    Ph <<= 1; Mh <<= 1;
    if (hin > 0) Ph |= 1ull; else if (hin < 0) Mh |= 1ull;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

// the same step on a 32-bit word, without branches (rtk_myers_fast32)
RTK_DEV int rtk_myers_step32(uint32_t& Pv, uint32_t& Mv, uint32_t Eq, int hin, int bit, uint32_t& Ph_out, uint32_t& Mh_out) {
    const uint32_t pv = Pv, mv = Mv;
    const uint32_t Xv = Eq | mv;
    Eq |= static_cast<uint32_t>(hin) >> 31; // hin < 0
    const uint32_t Xh = (((Eq & pv) + pv) ^ pv) | Eq;
    uint32_t Ph = mv | ~(Xh | pv);
    uint32_t Mh = pv & Xh;
    Ph_out = Ph; Mh_out = Mh;
    const int hout = static_cast<int>((Ph >> bit) & 1u) - static_cast<int>((Mh >> bit) & 1u);
    Ph = (Ph << 1) | (hin > 0 ? 1u : 0u); Mh = (Mh << 1) | (static_cast<uint32_t>(hin) >> 31);
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    return hout;
}

// Query profile: peq[cls * W + w], bit i of word w set iff query[64w+i] equals a character of class cls.
RTK_FN void rtk_myers_build_peq(const MyersScratch& sc, MySeq q, int W, bool iupac) {
    for (int w = rtk_lane(); w < W; w += RTK_WAVE) {
        uint64_t acc[15];
        for (int c = 0; c < 15; ++c) acc[c] = 0;
        const int lim = (q.n - 64 * w) < 64 ? (q.n - 64 * w) : 64;
        for (int i = 0; i < lim; ++i) {
            uint32_t m = rtk_eq_classes(rtk_cls(rtk_seq_at(q, 64 * w + i)), iupac);
            for (int c = 0; c < 15; ++c) acc[c] |= static_cast<uint64_t>((m >> c) & 1u) << i;
        }
        for (int c = 0; c < 15; ++c) sc.peq[static_cast<uint64_t>(c) * W + w] = acc[c];
    }
    rtk_sync();
}

RTK_DEV uint64_t rtk_myers_eq_word(const MyersScratch& sc, const MySeq& q, int W, int w, unsigned char tc) {
    const int cls = rtk_cls(tc);
    if (cls < 15) return sc.peq[static_cast<uint64_t>(cls) * W + w];
    uint64_t e = 0; // a byte outside the IUPAC alphabet only equals itself
    const int lim = (q.n - 64 * w) < 64 ? (q.n - 64 * w) : 64;
    for (int i = 0; i < lim; ++i) e |= static_cast<uint64_t>(rtk_seq_at(q, 64 * w + i) == tc) << i;
    return e;
}

RTK_DEV unsigned char rtk_job_qc(const char* __restrict__ qp, int m, int qrev, int i) { return static_cast<unsigned char>(qrev ? qp[m - 1 - i] : qp[i]); }
RTK_DEV void rtk_myers_eq4(const char* __restrict__ qp, int m, int qrev, int w, bool iupac, uint64_t& eqA, uint64_t& eqC, uint64_t& eqG, uint64_t& eqT) {
    eqA = 0; eqC = 0; eqG = 0; eqT = 0;
    const int lim = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
    for (int i = 0; i < lim; ++i) {
        const unsigned char qc = rtk_job_qc(qp, m, qrev, 64 * w + i);
        uint32_t bm;
        if (qc == 'A') bm = 1u; else if (qc == 'C') bm = 2u; else if (qc == 'G') bm = 4u; else if (qc == 'T') bm = 8u;
        else bm = rtk_eq_classes(rtk_cls(qc), iupac) & 0xFu; // bases this query character equals
        eqA |= static_cast<uint64_t>(bm & 1u) << i; eqC |= static_cast<uint64_t>((bm >> 1) & 1u) << i;
        eqG |= static_cast<uint64_t>((bm >> 2) & 1u) << i; eqT |= static_cast<uint64_t>((bm >> 3) & 1u) << i;
    }
}
#endif
