// Unit-cost global (NW) edit distance of two byte strings on the host: exact, no cap. Written for rtk_identity's plain route ([A19]) as the
// independent restatement the device's aligner is held to: it shares nothing with csrc/hip or oracle/.
// Method: Myers' bit-vector recurrence in Hyyro's block form -- the query in words of 64 rows, one (Pv, Mv) pair of vertical deltas per word, a column at a time,
// the horizontal delta handed from a word to the one below it -- restricted to the Ukkonen band of a bound k: an alignment of cost <= k never leaves the diagonals
// [min(d, 0) - h, max(d, 0) + h], d = n - m, h = (k - |d|) / 2. Only the words that hold a row of the band at column j are computed. A word that enters the band
// at the bottom starts with deltas of +1 under the score of the word above it, and the word at the top of the band takes +1 from the row above it: both are upper
// bounds of the true scores, so every score computed is that of a real alignment and >= the distance, and a score <= k is the distance. A score above k widens the
// band (the part of k beyond |d| doubles, never beyond the score just found, which is itself a bound) and the pass runs again.
// Two bytes are equal iff identical: callers fold case before they call.
#ifndef RTK_COMMON_EDIT_DISTANCE_HPP
#define RTK_COMMON_EDIT_DISTANCE_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtk {

class EditDistance { // (keeps its buffers from call to call: one per thread)
public:
    uint64_t passes = 0; // banded passes run so far (a pair costs one, plus one per widening)

    // distance of q[0 .. m) and t[0 .. n); the first bound tried is |n - m| + 64
    int64_t operator()(const char* q, size_t m, const char* t, size_t n) {
        if (m == 0 || n == 0) return static_cast<int64_t>(m > n ? m : n);
        const int64_t M = static_cast<int64_t>(m), N = static_cast<int64_t>(n), W = (M + 63) >> 6, ad = N > M ? N - M : M - N;
        // the profile: for every byte that occurs in q, one bit per row
        for (int c = 0; c < 256; ++c) sym_[c] = -1;
        int n_sym = 0;
        for (int64_t i = 0; i < M; ++i) { const unsigned char c = static_cast<unsigned char>(q[i]); if (sym_[c] < 0) sym_[c] = n_sym++; }
        peq_.assign(static_cast<size_t>(n_sym) * static_cast<size_t>(W), 0);
        for (int64_t i = 0; i < M; ++i) peq_[static_cast<size_t>(sym_[static_cast<unsigned char>(q[i])]) * static_cast<size_t>(W) + static_cast<size_t>(i >> 6)] |= 1ull << (i & 63);
        pv_.resize(static_cast<size_t>(W)); mv_.resize(static_cast<size_t>(W)); score_.resize(static_cast<size_t>(W));
        int64_t k = ad + 64;
        for (;;) {
            const int64_t s = pass(reinterpret_cast<const unsigned char*>(t), M, N, k);
            if (s <= k) return s;
            const int64_t wider = ad + 2 * (k - ad > 0 ? k - ad : 1);
            k = wider < s ? wider : s;
        }
    }

private:
    int sym_[256];
    std::vector<uint64_t> peq_, pv_, mv_;
    std::vector<int64_t> score_; // score at the last row of a word, in the column just computed

    // one word, one column: the deltas of the word move on by a column; returns the horizontal delta that leaves the word at row `bit`
    static inline int step(uint64_t& Pv, uint64_t& Mv, uint64_t Eq, int hin, int bit) {
        const uint64_t neg = hin < 0 ? 1ull : 0ull;
        const uint64_t Xv = Eq | Mv;
        Eq |= neg;
        const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint64_t Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
        const int hout = static_cast<int>((Ph >> bit) & 1ull) - static_cast<int>((Mh >> bit) & 1ull);
        Ph <<= 1; Mh <<= 1;
        Mh |= neg; if (hin > 0) Ph |= 1ull;
        Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
        return hout;
    }

    // the score of the last cell when only the band of k is computed (>= the distance; equal to it when <= k)
    int64_t pass(const unsigned char* t, int64_t M, int64_t N, int64_t k) {
        ++passes;
        const int64_t W = (M + 63) >> 6, d = N - M, ad = d < 0 ? -d : d, h = k > ad ? (k - ad) / 2 : 0;
        const int64_t dlo = (d < 0 ? d : 0) - h, dhi = (d > 0 ? d : 0) + h; // rows j - dhi .. j - dlo of column j
        const int last_bit = static_cast<int>((M - 1) & 63);
        int64_t first = 0, last = -1;
        for (int64_t j = 0; j < N; ++j) {
            const int64_t top = j - dhi, bottom = j - dlo;
            first = top > 0 ? top >> 6 : 0;
            const int64_t nl = (bottom >> 6) < W - 1 ? (bottom >> 6) : W - 1;
            while (last < nl) { // a word enters at the bottom: +1 per row under the word above it, as of the column before this one
                ++last;
                const int64_t rows = last == W - 1 ? M - 64 * last : 64;
                pv_[static_cast<size_t>(last)] = ~0ull; mv_[static_cast<size_t>(last)] = 0;
                score_[static_cast<size_t>(last)] = (last == 0 ? j : score_[static_cast<size_t>(last - 1)]) + rows;
            }
            const int id = sym_[t[j]];
            const uint64_t* eq = id >= 0 ? &peq_[static_cast<size_t>(id) * static_cast<size_t>(W)] : nullptr;
            int hin = 1; // the top row of the matrix, or the bound above the band
            for (int64_t w = first; w <= last; ++w) {
                hin = step(pv_[static_cast<size_t>(w)], mv_[static_cast<size_t>(w)], eq ? eq[w] : 0ull, hin, w == W - 1 ? last_bit : 63);
                score_[static_cast<size_t>(w)] += hin;
            }
        }
        return score_[static_cast<size_t>(W - 1)]; // (the last word holds a row of the band at the last column: dlo <= n - m)
    }
};

} // namespace rtk

#endif
