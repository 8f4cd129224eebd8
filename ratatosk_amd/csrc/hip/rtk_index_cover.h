// rtk_index_cover_*: the crossings of low-coverage edges by the text of other sequences (k_cover_map) -- the device side of the last block of the reference's
// first-pass addCoverage, "Covering low coverage edges." (src/Graph.cpp:3085-3363; DESIGN.md section 4 [A16]; the rule and the host routes: tools/index/cover.hpp).
// The reference maps every sequence of the k2 unitig file onto the k1 graph and, wherever two consecutive mappings are adjacent in the text and the edge between
// their unitigs was recorded as shared by fewer than min_cov_vertices colours, gives both unitigs two fresh colour ids and clears the record. The search is done
// here, per text position; testing and clearing the records and handing out the ids depends on the order of the file and stays with the caller.
//   begin  unitig u = seq_pool[seq_off[u] .. seq_off[u + 1]); packed to 2 bits with its k-mer table in HBM, as the colour job does (DeviceUnitigs, rtk_index_colour.h);
//          low_bits[u]: the recorded edges of unitig u, bit idx(c) (A, C, G, T = 1, 2, 4, 8) for the successor of its forward strand that appends c, the same
//          bit << 4 for the successors of its reverse strand.
//   chunk  chars: pieces of sequences separated by '\n' (n_chars characters, at most 64 MB and 4 M pieces); piece r starts at starts[r] (starts[0] = 0, ascending), is
//          part of sequence seq_numbers[r] and begins at position first_positions[r] of it. A sequence longer than a chunk is cut so that every pair of windows
//          (p, p + 1), k + 1 characters, lies whole inside one piece: a piece starts k characters before the end of the one before it.
//   end    *crossings: two words each, ascending by the first (the order of the file, left to right); *n of them. Freed with rtk_free. The job is gone afterwards.
// A crossing is a position p of a sequence such that the k characters at p and the k at p + 1 are all A/C/G/T (either case), the k-mer at p is the LAST k-mer of its
// unitig u in the direction the text walks it, the k-mer at p + 1 is in the graph (on v; v may be u: a unitig that meets itself), and the recorded bit of u for
// (direction, character p + k) is set. Bits are only read here. Two words:
//   word 0 = sequence number << 32 | p                          (sequence numbers and positions below 2^32: a longer sequence is refused)
//   word 1 = u << 33 | v << 3 | direction << 2 | base           (direction 1: u is walked on its reverse strand; base: code of character p + k; unitigs below 2^30)
// Survivors are few (only low-coverage edges pass); the buffer has a counted capacity all the same (RTK_INDEX_COVER_CAP, tests: 1): a chunk whose survivors do not
// fit is mapped a second time into a buffer of the size it asked for.
#ifndef RTK_INDEX_COVER_H
#define RTK_INDEX_COVER_H
#include <string.h>
#include <cstdio>
#include <mutex>
#include <stdexcept>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "rtk_index_colour.h"
#include "rtk_index_common.h"

namespace {
#define RTK_COVER_MAX_UNITIGS (1ull << 30)
#define RTK_COVER_MAX_CHUNK (64ull << 20)

// One lane per character position of a chunk. Whole waves take part in every round: the survivors of a wave are appended with one atomic.
template <class KM>
__global__ void k_cover_map(const char* __restrict__ chars, uint64_t n, int k, const uint64_t* __restrict__ starts, const uint32_t* __restrict__ seq_numbers,
                            const uint64_t* __restrict__ first_positions, uint32_t n_seqs, GraphView g, const uint8_t* __restrict__ low,
                            uint64_t* __restrict__ keys, uint64_t* __restrict__ vals, unsigned long long* __restrict__ top, uint64_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        KM a = 0; uint32_t last = 0; bool ok = i + static_cast<uint64_t>(k) + 1 <= n; // the k + 1 characters of the two windows: a separator among them ends the pair
        if (ok) for (int j = 0; j <= k; ++j) { const uint32_t c = idx_code(static_cast<unsigned char>(chars[i + j])); ok = ok && c < 4u; if (j < k) a = (a << 2) | static_cast<KM>(c & 3u); else last = c & 3u; }
        bool keep = false; uint64_t w1 = 0;
        if (ok) {
            const ColPlace pa = col_place(g, a, k);
            if (pa.u != 0xFFFFFFFFu) {
                const uint64_t n_km = g.uoff[pa.u + 1] - g.uoff[pa.u] - static_cast<uint64_t>(k) + 1;
                const bool at_end = pa.fw ? static_cast<uint64_t>(pa.off) + 1 == n_km : pa.off == 0u; // the last k-mer of its unitig in the direction of travel
                const uint32_t bit = (1u << last) << (pa.fw ? 0 : 4);
                if (at_end && (static_cast<uint32_t>(low[pa.u]) & bit)) {
                    const KM b = ((a << 2) | static_cast<KM>(last)) & idx_kmask<KM>(k);
                    const ColPlace pb = col_place(g, b, k);
                    if (pb.u != 0xFFFFFFFFu) { keep = true; w1 = (static_cast<uint64_t>(pa.u) << 33) | (static_cast<uint64_t>(pb.u) << 3) | (pa.fw ? 0ull : 4ull) | last; }
                }
            }
        }
        const uint64_t keepers = __ballot(keep ? 1 : 0);
        if (!keepers) continue;
        const unsigned long long base = __shfl(lane == 0 ? atomicAdd(top, static_cast<unsigned long long>(__popcll(keepers))) : 0ull, 0, 64);
        if (keep) {
            const uint64_t at = base + static_cast<uint64_t>(__popcll(keepers & ((1ull << lane) - 1ull)));
            if (at < cap) {
                uint32_t lo = 0, hi = n_seqs; // the piece of position i: the last one that starts at or before it
                while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (starts[mid] <= i) lo = mid; else hi = mid; }
                keys[at] = (static_cast<uint64_t>(seq_numbers[lo]) << 32) | (first_positions[lo] + (i - starts[lo]));
                vals[at] = w1;
            }
        }
    }
}

struct CoverJob {
    int device = 0, k = 31; uint32_t n_unitigs = 0; DeviceUnitigs du;
    DevArr<uint8_t> low; DevArr<uint64_t> keys, vals; DevArr<unsigned long long> top;
    uint64_t cap = 0, n_found = 0; // n_found: the survivors of the chunks so far (the counter on the device says the same between two chunks)
    DevArr<char> d_chars; DevArr<uint64_t> d_starts, d_first; DevArr<uint32_t> d_seq; PinArr<char> h_chars; PinArr<uint64_t> h_starts, h_first; PinArr<uint32_t> h_seq; uint64_t chars_room = 0, seqs_room = 0;
    Stream st; std::mutex m; uint64_t bases = 0, chunks = 0, second_rounds = 0; double t_table = 0.0; StageClock clk;

    void begin(int device_, int k_, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs_, const uint8_t* low_bits) {
        device = device_; k = k_; n_unitigs = static_cast<uint32_t>(n_unitigs_);
        du.build(k, n_unitigs, seq_pool, seq_off);
        low.alloc(n_unitigs); rtk_check(hipMemcpy(low.p, low_bits, n_unitigs, hipMemcpyHostToDevice), "hipMemcpy");
        top.alloc(1); rtk_check(hipMemset(top.p, 0, 8), "hipMemset");
        cap = rtk_knob_index_cover_cap(1ull << 20); if (cap < 1) cap = 1;
        keys.alloc(cap); vals.alloc(cap);
        st.create();
        t_table = clk.since();
    }
    // room for a chunk of n_chars characters in n_seqs pieces (the buffers grow to the largest chunk seen)
    void make_room(uint64_t n_chars, uint64_t n_seqs) {
        if (n_chars > chars_room) { d_chars.alloc(n_chars); h_chars.alloc(n_chars); chars_room = n_chars; }
        if (n_seqs > seqs_room) { d_starts.alloc(n_seqs); d_first.alloc(n_seqs); d_seq.alloc(n_seqs); h_starts.alloc(n_seqs); h_first.alloc(n_seqs); h_seq.alloc(n_seqs); seqs_room = n_seqs; }
    }
    // the survivors so far moved into buffers of new_cap pairs
    void grow(uint64_t new_cap) {
        DevArr<uint64_t> k2, v2; k2.alloc(new_cap); v2.alloc(new_cap);
        if (n_found) { rtk_check(hipMemcpy(k2.p, keys.p, 8 * n_found, hipMemcpyDeviceToDevice), "hipMemcpy"); rtk_check(hipMemcpy(v2.p, vals.p, 8 * n_found, hipMemcpyDeviceToDevice), "hipMemcpy"); }
        std::swap(keys.p, k2.p); std::swap(vals.p, v2.p); cap = new_cap;
    }
    template <class KM> void map(uint64_t n_chars, uint32_t n_seqs) {
        launch("k_cover_map", k_cover_map<KM>, idx_grid(n_chars, 4096), st, d_chars.p, n_chars, k, d_starts.p, d_seq.p, d_first.p, n_seqs, du.g, low.p, keys.p, vals.p, top.p, cap);
    }
    uint64_t mapped(uint64_t n_chars, uint32_t n_seqs) { // the chunk on the device mapped; the counter afterwards
        by_key_type(k, [&](auto km) { map<decltype(km)>(n_chars, n_seqs); return 0; });
        rtk_check(hipStreamSynchronize(st), "k_cover_map");
        return read_word(top.p);
    }
    void chunk(const char* chars, uint64_t n_chars, const uint64_t* starts, const uint32_t* seq_numbers, const uint64_t* first_positions, uint32_t n_seqs) {
        make_room(n_chars, n_seqs);
        memcpy(h_chars.p, chars, n_chars); memcpy(h_starts.p, starts, 8ull * n_seqs); memcpy(h_seq.p, seq_numbers, 4ull * n_seqs); memcpy(h_first.p, first_positions, 8ull * n_seqs);
        rtk_check(hipMemcpyAsync(d_chars.p, h_chars.p, n_chars, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_starts.p, h_starts.p, 8ull * n_seqs, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_seq.p, h_seq.p, 4ull * n_seqs, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_first.p, h_first.p, 8ull * n_seqs, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        uint64_t n = mapped(n_chars, n_seqs);
        if (n > cap) { // second round: the chunk is still on the device; what it wrote below the old capacity is written again to the same places or others, all of it kept
            ++second_rounds;
            grow(std::max<uint64_t>(n, 2 * cap));
            rtk_check(hipMemcpy(top.p, &n_found, 8, hipMemcpyHostToDevice), "hipMemcpy");
            n = mapped(n_chars, n_seqs);
            if (n > cap) throw std::runtime_error("the second round of a chunk found more crossings than the first");
        }
        n_found = n; bases += n_chars; ++chunks;
    }
    // the crossings sorted by their first word, two words each; false: out of host memory
    bool end(HostOut<uint64_t>& out) {
        if (!out.alloc(2 * n_found)) return false;
        if (n_found == 0) return true;
        DevArr<uint64_t> k2, v2; DevArr<char> tmp; k2.alloc(n_found); v2.alloc(n_found);
        rocprim::double_buffer<uint64_t> dk(keys.p, k2.p), dv(vals.p, v2.p);
        prim(tmp, "rocprim::radix_sort_pairs", [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, dk, dv, n_found, 0, 64); });
        std::vector<uint64_t> hk(n_found), hv(n_found);
        rtk_check(hipMemcpy(hk.data(), dk.current(), 8 * n_found, hipMemcpyDeviceToHost), "hipMemcpy"); rtk_check(hipMemcpy(hv.data(), dv.current(), 8 * n_found, hipMemcpyDeviceToHost), "hipMemcpy");
        for (uint64_t i = 0; i < n_found; ++i) { out.p[2 * i] = hk[i]; out.p[2 * i + 1] = hv[i]; }
        return true;
    }
    void trace_end() {
        if (clk.trace) fprintf(stderr, "rtk_index_cover: %llu characters in %llu chunks -> %llu crossings of recorded edges (%llu chunks mapped a second time); table %.2f s, all %.2f s\n", static_cast<unsigned long long>(bases),
                               static_cast<unsigned long long>(chunks), static_cast<unsigned long long>(n_found), static_cast<unsigned long long>(second_rounds), t_table, clk.since());
    }
};
} // namespace
#endif
