// The nucleotide alphabet on the device: character classes (A C G T, the 11 IUPAC codes, anything else), which classes count as equal
// (reference: src/Common.hpp:262-276), and the branch-free 2-bit packing of A/C/G/T text into k-mer codes.
#ifndef RTK_ACGT_H
#define RTK_ACGT_H
#include "rtk_wave.h"

// character class: 0..3 A C G T, 4..14 M R S V W Y H K D B N, 15 anything else
RTK_DEV int rtk_cls(unsigned char c) {
    switch (c) {
        case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3;
        case 'M': return 4; case 'R': return 5; case 'S': return 6; case 'V': return 7; case 'W': return 8; case 'Y': return 9;
        case 'H': return 10; case 'K': return 11; case 'D': return 12; case 'B': return 13; case 'N': return 14;
        default: return 15;
    }
}

// 15-bit set of classes a character of class c is equal to (identity + the 28 (code, base) pairs of Common.hpp:262-274)
RTK_DEV uint32_t rtk_eq_classes(int c, bool iupac) {
    if (c >= 15) return 0u;
    uint32_t m = 1u << c;
    if (!iupac) return m;
    // base sets of the codes:           M    R    S    V    W    Y    H     K     D     B     N
    const uint32_t code_set[11] = {0x3, 0x5, 0x6, 0x7, 0x9, 0xA, 0xB, 0xC, 0xD, 0xE, 0xF};
    if (c < 4) { for (int i = 0; i < 11; ++i) if ((code_set[i] >> c) & 1u) m |= 1u << (4 + i); }
    else m |= code_set[c - 4];
    return m;
}

RTK_DEV bool rtk_chars_equal(unsigned char a, unsigned char b, bool iupac) {
    if (a == b) return true;
    const int ca = rtk_cls(a), cb = rtk_cls(b);
    if (ca >= 15 || cb >= 15) return false;
    return (rtk_eq_classes(ca, iupac) >> cb) & 1u;
}

// Branch-free 2-bit packing of up to 32 characters (A 0, C 1, G 2, T 3; first character in the high bits of the result, `want`
// characters in total, unaligned source with at least 32 readable bytes). *n_ok = number of leading characters that are A/C/G/T
// (upper case), capped at `want`; the code is only meaningful for those. Bits 1-2 of 'A' 0x41, 'C' 0x43, 'T' 0x54, 'G' 0x47 are a
// 2-bit code; a character is valid iff rebuilding it from that code gives it back. No per-character branches: the per-lane switch
// of rtk_cls costs ~50 scalar instructions per character in exec-mask bookkeeping.
RTK_DEV uint64_t rtk_spread8(uint64_t v) { v = (v | (v << 4)) & 0x0F0Full; v = (v | (v << 2)) & 0x3333ull; return (v | (v << 1)) & 0x5555ull; } // bit i of a byte -> bit 2i
// inv2 (optional): bit 2(want-1-i) set iff character i is not A/C/G/T (same layout as the low code bits)
RTK_DEV uint64_t rtk_pack_acgt(const unsigned char* p, int want, int* n_ok, uint64_t* inv2 = nullptr) {
    uint64_t code = 0, inv = 0; int ok = 0; bool open = true;
    for (int j = 0; j < 4; ++j) {
        uint64_t x; __builtin_memcpy(&x, p + 8 * j, 8);
        const uint64_t b1 = (x >> 1) & 0x0101010101010101ull, b2 = (x >> 2) & 0x0101010101010101ull;
        const uint64_t b12 = b1 & b2, b2n = b2 & ~b1;
        const uint64_t recon = 0x4141414141414141ull + (b1 << 1) + (b12 << 2) + (b2n << 4) + (b2n << 1) + b2n;
        const uint64_t bad = x ^ recon;
        const int good = bad ? (__builtin_ctzll(bad) >> 3) : 8; // leading valid characters of this word
        // gather the bit planes, first character first: byte i -> bit 7 - i
        const uint64_t hi = (b2 * 0x8040201008040201ull) >> 56, lo = ((b1 ^ b2) * 0x8040201008040201ull) >> 56;
        code = (code << 16) | (rtk_spread8(hi) << 1) | rtk_spread8(lo);
        if (inv2) {
            const uint64_t nz = ((((bad & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | bad) >> 7) & 0x0101010101010101ull; // 1 per non-zero byte
            inv = (inv << 16) | rtk_spread8((nz * 0x8040201008040201ull) >> 56);
        }
        if (open) { ok += good; open = good == 8; }
    }
    // 32 characters packed; keep the first `want`
    if (want < 32) { code >>= 2 * (32 - want); inv >>= 2 * (32 - want); }
    if (inv2) *inv2 = inv;
    *n_ok = ok < want ? ok : want;
    return code;
}

// the k-mer code (k <= 63) of the k characters at p; false when one of them is not A/C/G/T. Reads at most max(32, k) bytes from p.
RTK_DEV bool rtk_km_from_text(const unsigned char* p, int k, RtkKm* out) {
    int n_ok;
    if (k <= 32) { out->hi = 0; out->lo = rtk_pack_acgt(p, k, &n_ok); return n_ok == k; }
    out->hi = rtk_pack_acgt(p, k - 32, &n_ok);
    if (n_ok != k - 32) return false;
    out->lo = rtk_pack_acgt(p + (k - 32), 32, &n_ok);
    return n_ok == 32;
}
#endif
