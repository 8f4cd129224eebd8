// Rescue of unmapped short reads before the index build (`correct -u`; reference: retrieveMissingReads, src/Graph.cpp:3857-4131, called at src/Ratatosk.cpp:1040-1056).
// The reference keeps a read of the `-u` files when enough of its k1-mers are in the long reads and not in the `-s` reads, both sets held in Bloom filters.
// Here the sets are exact ([A11]): LR2 / SR2 = the canonical k-mers seen at least twice in the long / the `-s` reads, as rtk_index_count_kmers
// returns them; D = LR2 \ SR2; a read qualifies when at least `min_positions` of its start positions spell a k-mer of D.
//   rtk_rescue_begin   D formed on the device (one lane per k-mer of LR2, bisection in SR2) and inserted into an open-addressing table of 8-byte keys in HBM
//   rtk_rescue_chunk   k_rescue: a wave owns whole reads, 64 start positions per step, one probe of D per position, one byte per read written
//   rtk_rescue_end     the two counters of the job; releases it
// One-word k-mers only (odd k <= 31). HBM-bound on the text (1 byte per position) plus one 8-byte slot (rarely more) per position whose window is all A/C/G/T.
#include <string.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>

#include "rtk_index_common.h" // the owners, launch and entry helpers of the index build's device side
#include "rtk_kmer_window.h"  // rsc_code / rsc_spread / rsc_window / rsc_slot, shared with rtk_qv.hip

namespace {

__device__ __forceinline__ bool rsc_in_sorted(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n; // first element >= x
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo < n && a[lo] == x;
}

__global__ void k_rescue_fill(uint64_t* __restrict__ T, uint64_t slots) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < slots; i += stride) T[i] = RTK_RESCUE_EMPTY;
}
// D = LR2 \ SR2, one lane per k-mer of LR2. T == nullptr: the members are counted (one atomic per wave); else they are inserted (distinct keys, a table
// that nothing reads before this kernel is over).
__global__ void k_rescue_diff(const uint64_t* __restrict__ lr, uint64_t n_lr, const uint64_t* __restrict__ sr, uint64_t n_sr, uint64_t* __restrict__ T, uint64_t slots, unsigned long long* __restrict__ n_d) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n_lr; i0 += stride) { // (whole waves take part in every round)
        const uint64_t i = i0 + threadIdx.x;
        const uint64_t x = i < n_lr ? lr[i] : 0;
        const bool in_d = i < n_lr && !rsc_in_sorted(sr, n_sr, x);
        if (!T) {
            const uint64_t bal = __ballot(in_d ? 1 : 0);
            if (bal && (threadIdx.x & 63) == 0) atomicAdd(n_d, static_cast<unsigned long long>(__popcll(bal)));
        } else if (in_d) {
            uint64_t s = rsc_slot(x, slots);
            while (atomicCAS(reinterpret_cast<unsigned long long*>(T + s), static_cast<unsigned long long>(RTK_RESCUE_EMPTY), static_cast<unsigned long long>(x)) != RTK_RESCUE_EMPTY) s = s + 1 == slots ? 0 : s + 1;
        }
    }
}

// A wave takes read after read of the chunk (sequences separated by '\n'; read r = chars[starts[r] .. starts[r + 1]), the last one up to n). Per step it looks at 64
// start positions: every lane loads the character of its position and one of the k - 1 that follow the tile, three ballots per half turn them into bit planes (low
// bit, high bit, not A/C/G/T) of 128 characters, and a lane's window is k bits of each plane from its own position on -- no loop over the k characters, no branch.
// The planes hold the first base in the LOWEST bit, the k-mer code wants it in the highest: interleaved as they are they spell the window backwards, whose complement is the
// reverse complement; the forward code is the reverse complement of that. Windows that are all A/C/G/T probe D; hits are counted per read with a ballot, the
// counter is wave-uniform. counters[0] += positions probed, counters[1] += hits: one atomic instruction per wave, at its end.
__global__ void k_rescue(const char* __restrict__ chars, uint64_t n, const uint64_t* __restrict__ starts, uint32_t n_reads, int k, uint32_t min_positions,
                         const uint64_t* __restrict__ T, uint64_t slots, unsigned char* __restrict__ keep, unsigned long long* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = rtk_u((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = rtk_u((gridDim.x * blockDim.x) >> 6);
    const uint64_t wmask = (1ull << k) - 1ull, kmask = (1ull << (2 * k)) - 1ull;
    uint64_t n_probed = 0, n_hits = 0;
    for (uint32_t r = wave; r < n_reads; r += n_waves) {
        uint64_t end = rtk_u(r + 1u < n_reads ? starts[r + 1u] : n); if (end > n) end = n;
        uint64_t beg = rtk_u(starts[r]); if (beg > end) beg = end;
        uint32_t cnt = 0;
        for (uint64_t t = beg; t + static_cast<uint64_t>(k) <= end; t += 64) {
            const uint64_t i0 = t + static_cast<uint64_t>(lane), i1 = i0 + 64;
            const uint32_t c0 = i0 < end ? rsc_code(static_cast<unsigned char>(chars[i0])) : 4u;
            const uint32_t c1 = (lane < k - 1 && i1 < end) ? rsc_code(static_cast<unsigned char>(chars[i1])) : 4u;
            const uint64_t lo0 = __ballot(c0 & 1u), hi0 = __ballot(c0 & 2u), bad0 = __ballot(c0 >> 2), lo1 = __ballot(c1 & 1u), hi1 = __ballot(c1 & 2u), bad1 = __ballot(c1 >> 2);
            const bool ok = (rsc_window(bad0, bad1, lane) & wmask) == 0; // (the separator and everything behind the read are not bases: no window reaches into the next read)
            const uint64_t back = rsc_spread(rsc_window(lo0, lo1, lane) & wmask) | (rsc_spread(rsc_window(hi0, hi1, lane) & wmask) << 1);
            const uint64_t rc = ~back & kmask, fw = rtk_revcomp(rc, k), can = fw <= rc ? fw : rc;
            bool hit = false;
            if (ok) {
                uint64_t s = rsc_slot(can, slots);
                for (uint64_t tries = 0; tries < slots; ++tries) { const uint64_t key = T[s]; if (key == can) { hit = true; break; } if (key == RTK_RESCUE_EMPTY) break; s = s + 1 == slots ? 0 : s + 1; }
            }
            n_probed += static_cast<uint64_t>(__popcll(__ballot(ok ? 1 : 0)));
            cnt += static_cast<uint32_t>(__popcll(__ballot(hit ? 1 : 0)));
        }
        n_hits += cnt;
        if (lane == 0) keep[r] = cnt >= min_positions ? 1 : 0;
    }
    if (lane < 2 && (n_probed | n_hits)) atomicAdd(counters + lane, static_cast<unsigned long long>(lane == 0 ? n_probed : n_hits));
}

struct Rescue { static const char* dev() { return "hipMalloc (rescue)"; } static const char* pin() { return "hipHostMalloc (rescue)"; } };
template <class T> using RscDev = DevArr<T, Rescue>;
template <class T> using RscPin = PinArr<T, Rescue>;

struct RescueJob {
    int device = 0, k = 31; uint32_t min_positions = 31;
    RscDev<uint64_t> table; RscDev<unsigned long long> counters; uint64_t slots = 0, n_d = 0; // counters: positions probed, hits, |D|
    // two chunks in flight (callers on two threads overlap the copies of one with the kernel of the other); a slot is one caller's from its copy in to its copy out
    RscDev<char> d_chars[2]; RscDev<uint64_t> d_starts[2]; RscDev<unsigned char> d_keep[2]; RscPin<char> h_chars[2]; RscPin<uint64_t> h_starts[2]; RscPin<unsigned char> h_keep[2];
    Stream st[2]; std::mutex m[2]; std::atomic<unsigned> next{0};
    std::atomic<uint64_t> chars{0}, chunks{0}; double t_table = 0.0; StageClock clk;

    // D = the long-read k-mers that are no short-read k-mers, counted and then inserted into the table
    void build_table(const uint64_t* lr, uint64_t n_lr, const uint64_t* sr, uint64_t n_sr) {
        counters.alloc(3); rtk_check(hipMemset(counters.p, 0, 24), "hipMemset");
        unsigned long long* d_nd = counters.p + 2;
        RscDev<uint64_t> d_lr, d_sr; d_lr.alloc(n_lr); d_sr.alloc(n_sr); // released when D exists
        if (n_lr) rtk_check(hipMemcpy(d_lr.p, lr, 8 * n_lr, hipMemcpyHostToDevice), "hipMemcpy");
        if (n_sr) rtk_check(hipMemcpy(d_sr.p, sr, 8 * n_sr, hipMemcpyHostToDevice), "hipMemcpy");
        if (n_lr) { launch("k_rescue_diff", k_rescue_diff, idx_grid(n_lr), 0, d_lr.p, n_lr, d_sr.p, n_sr, nullptr, 0ull, d_nd); rtk_check(hipDeviceSynchronize(), "k_rescue_diff"); }
        n_d = read_word(d_nd); slots = 2 * n_d + 64; // load <= 0.5: a probe ends in its first slot more often than not
        table.alloc(slots);
        launch("k_rescue_fill", k_rescue_fill, idx_grid(slots), 0, table.p, slots);
        if (n_d) launch("k_rescue_diff", k_rescue_diff, idx_grid(n_lr), 0, d_lr.p, n_lr, d_sr.p, n_sr, table.p, slots, d_nd);
        rtk_check(hipDeviceSynchronize(), "rescue table");
    }
    void begin(int device_, int k_, const uint64_t* lr, uint64_t n_lr, const uint64_t* sr, uint64_t n_sr, uint32_t min_positions_) {
        device = device_; k = k_; min_positions = min_positions_;
        build_table(lr, n_lr, sr, n_sr);
        for (int i = 0; i < 2; ++i) {
            d_chars[i].alloc(RTK_RESCUE_CHUNK); d_starts[i].alloc(RTK_RESCUE_READS); d_keep[i].alloc(RTK_RESCUE_READS);
            h_chars[i].alloc(RTK_RESCUE_CHUNK); h_starts[i].alloc(RTK_RESCUE_READS); h_keep[i].alloc(RTK_RESCUE_READS);
            st[i].create();
        }
        t_table = clk.since();
        if (clk.trace) fprintf(stderr, "rtk_rescue_begin: %llu long-read k-mers, %llu short-read k-mers -> %llu in the long reads only, table of %llu slots in %.2f s\n", static_cast<unsigned long long>(n_lr),
                               static_cast<unsigned long long>(n_sr), static_cast<unsigned long long>(n_d), static_cast<unsigned long long>(slots), t_table);
    }
    void chunk(const char* text, uint64_t n_chars, const uint64_t* starts, uint32_t n_reads, unsigned char* keep) {
        const int sl = static_cast<int>(next.fetch_add(1) & 1u);
        std::lock_guard<std::mutex> lk(m[sl]);
        memcpy(h_chars[sl].p, text, n_chars); memcpy(h_starts[sl].p, starts, 8ull * n_reads);
        rtk_check(hipMemcpyAsync(d_chars[sl].p, h_chars[sl].p, n_chars, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_starts[sl].p, h_starts[sl].p, 8ull * n_reads, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((static_cast<uint64_t>(n_reads) + 3) / 4, 2048)); // 4 waves per block, one read per wave and round
        launch("k_rescue", k_rescue, dim3(blocks), st[sl], d_chars[sl].p, n_chars, d_starts[sl].p, n_reads, k, min_positions, table.p, slots, d_keep[sl].p, counters.p);
        rtk_check(hipMemcpyAsync(h_keep[sl].p, d_keep[sl].p, n_reads, hipMemcpyDeviceToHost, st[sl]), "hipMemcpyAsync");
        rtk_check(hipStreamSynchronize(st[sl]), "k_rescue");
        memcpy(keep, h_keep[sl].p, n_reads);
        chars += n_chars; ++chunks;
    }
    void end(uint64_t* n_positions_probed, uint64_t* n_hits) {
        rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        unsigned long long c[2] = {0, 0}; rtk_check(hipMemcpy(c, counters.p, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_positions_probed = c[0]; *n_hits = c[1];
        if (clk.trace) fprintf(stderr, "rtk_rescue: %llu characters in %llu chunks, %llu positions probed, %llu hits; table %.2f s, all %.2f s\n", static_cast<unsigned long long>(chars.load()),
                               static_cast<unsigned long long>(chunks.load()), c[0], c[1], t_table, clk.since());
    }
};

} // namespace

extern "C" int rtk_rescue_begin(int device, int k, const uint64_t* lr, uint64_t n_lr, const uint64_t* sr, uint64_t n_sr, uint32_t min_positions, void** job_out) {
    if (!job_out || (!lr && n_lr) || (!sr && n_sr)) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_begin: null argument");
    if (k < 3 || k > 31 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_rescue_begin: odd k <= 31 only (one-word k-mers)");
    if (min_positions < 1) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_begin: min_positions must be at least 1");
    if (const int rc = check_device("rtk_rescue_begin", device)) return rc;
    *job_out = nullptr;
    for (uint64_t i = 1; i < n_lr; ++i) if (lr[i - 1] >= lr[i]) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_begin: the long-read k-mers are not sorted and distinct");
    for (uint64_t i = 1; i < n_sr; ++i) if (sr[i - 1] >= sr[i]) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_begin: the short-read k-mers are not sorted and distinct");
    return entry("rtk_rescue_begin", device, [&]() { std::unique_ptr<RescueJob> J(new RescueJob()); J->begin(device, k, lr, n_lr, sr, n_sr, min_positions); *job_out = J.release(); return RTK_OK; });
}

extern "C" int rtk_rescue_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_reads, unsigned char* keep) {
    RescueJob* J = static_cast<RescueJob*>(job);
    if (!J || !chars || !starts || !keep) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_chunk: null argument");
    if (n_reads == 0) return RTK_OK;
    if (n_chars > RTK_RESCUE_CHUNK || n_reads > RTK_RESCUE_READS) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_chunk: chunk larger than 64 MB of characters / 4 M reads");
    for (uint32_t r = 0; r < n_reads; ++r) if (starts[r] > n_chars || (r && starts[r] < starts[r - 1])) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_chunk: read starts must ascend and lie inside the chunk");
    return entry("rtk_rescue_chunk", J->device, [&]() { J->chunk(chars, n_chars, starts, n_reads, keep); return RTK_OK; });
}

extern "C" int rtk_rescue_end(void* job, uint64_t* n_positions_probed, uint64_t* n_hits) {
    std::unique_ptr<RescueJob> J(static_cast<RescueJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_rescue_end: null job");
    if (!n_positions_probed || !n_hits) return RTK_OK; // (abandoned job: released)
    *n_positions_probed = 0; *n_hits = 0;
    return entry("rtk_rescue_end", J->device, [&]() { J->end(n_positions_probed, n_hits); return RTK_OK; });
}
