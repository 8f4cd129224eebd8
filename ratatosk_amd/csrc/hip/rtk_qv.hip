// k-mer QV of reads against a set of k-mers (rtk_qv, `correct --qv`; DESIGN.md section 4, [A17]): of the start positions of a text whose k characters are all
// A/C/G/T, how many spell a canonical k-mer of the set. No counterpart in the reference: the figure is Merqury's, the set is what rtk_index_count_kmers returns.
//   rtk_qv_begin   the set inserted into an open-addressing table of 8-byte keys in HBM (the table of rtk_rescue.hip: load <= 0.5, all-ones = empty)
//   rtk_qv_chunk   k_qv: work cut by POSITION, not by read -- a wave takes span after span of RTK_QV_SPAN start positions of the chunk, whatever pieces they
//                  fall into, so that a read of a megabase costs what a thousand reads of a kilobase cost; two counts per piece
//   rtk_qv_end     the two totals of the job; releases it
// One-word k-mers only (odd k <= 31). HBM-bound on the text (1 byte per position) plus one 8-byte slot (rarely more) per valid window, as k_rescue.
#include <string.h>

#include <atomic>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>

#include "rtk_index_common.h" // the owners, launch and entry helpers of the index build's device side
#include "rtk_kmer_window.h"  // rsc_code / rsc_spread / rsc_window / rsc_slot and the table's constants, shared with rtk_rescue.hip

namespace {

// Start positions one wave takes at a time: 32 steps of 64. A span costs one search in `starts` and at least two atomics; a chunk of 64 MB has 32 Ki of them,
// four per wave of the largest grid, and a text of 1 MB still has 512, two waves for every CU.
#define RTK_QV_SPAN 2048u

// one lane per k-mer of the set (distinct keys, a table that nothing reads before this kernel is over)
__global__ void k_qv_insert(const uint64_t* __restrict__ solid, uint64_t n, uint64_t* __restrict__ T, uint64_t slots) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t x = solid[i];
        uint64_t s = rsc_slot(x, slots);
        while (atomicCAS(reinterpret_cast<unsigned long long*>(T + s), static_cast<unsigned long long>(RTK_RESCUE_EMPTY), static_cast<unsigned long long>(x)) != RTK_RESCUE_EMPTY) s = s + 1 == slots ? 0 : s + 1;
    }
}

// the wave's counts of piece p go to its two words: one lane, device-scope adds, nothing for a zero
__device__ __forceinline__ void qv_flush(int lane, uint32_t p, uint32_t cw, uint32_t cf, uint32_t* __restrict__ windows, uint32_t* __restrict__ found) {
    if (lane == 0) { if (cw) atomicAdd(windows + p, cw); if (cf) atomicAdd(found + p, cf); }
}

// The text of a chunk is pieces separated by '\n' (piece p = chars[starts[p] .. starts[p + 1]), the last one up to n; starts[0] = 0, ascending). A wave takes the
// spans wave, wave + n_waves, ... of RTK_QV_SPAN start positions each. The piece of a span's first position is the last one that starts at or before it: one
// search in `starts`, 64 probes a round. Then 64 positions per step with the bit-plane window of k_rescue (rtk_kmer_window.h); the planes of the 64 characters
// behind the step are the next step's own, so every character is loaded once. A window that holds a separator or any other non-base is invalid: no window
// reaches into the next piece, the text alone decides, and `starts` only says whose count a position is. The two counts of the current piece are wave-uniform;
// they are flushed when the piece changes and at the end of the span. A step that holds piece boundaries splits its two ballots there, boundary by boundary.
// totals[0] += valid windows, totals[1] += found: one atomic instruction per wave, at its end. All sums are integers: the order of the waves does not show.
__global__ void k_qv(const char* __restrict__ chars, uint64_t n, const uint64_t* __restrict__ starts, uint32_t n_pieces, int k, const uint64_t* __restrict__ T, uint64_t slots,
                     uint32_t* __restrict__ windows, uint32_t* __restrict__ found, unsigned long long* __restrict__ totals) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = rtk_u((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = rtk_u((gridDim.x * blockDim.x) >> 6);
    const uint64_t wmask = (1ull << k) - 1ull, kmask = (1ull << (2 * k)) - 1ull;
    const uint64_t n_spans = (n + RTK_QV_SPAN - 1) / RTK_QV_SPAN;
    uint64_t tot_w = 0, tot_f = 0;
    for (uint64_t span = wave; span < n_spans; span += n_waves) {
        const uint64_t pos0 = span * RTK_QV_SPAN, pos_end = pos0 + RTK_QV_SPAN < n ? pos0 + RTK_QV_SPAN : n;
        uint32_t p = 0, hi = n_pieces; // starts[p] <= pos0 < starts[hi] (starts[n_pieces]: never reached)
        while (hi - p > 1) {
            const uint32_t st = (hi - p + 63u) / 64u;
            const uint64_t q = static_cast<uint64_t>(p) + static_cast<uint64_t>(lane) * st;
            const uint64_t le = __ballot(q < hi && starts[q] <= pos0 ? 1 : 0); // (ascending starts: ones, then zeros; lane 0 is a one)
            p += static_cast<uint32_t>(__popcll(le) - 1) * st;
            if (hi - p > st) hi = p + st;
        }
        uint64_t next = p + 1u < n_pieces ? starts[p + 1u] : ~0ull; // where the piece after p starts
        uint32_t cw = 0, cf = 0;
        uint64_t lo0, hi0, bad0;
        { const uint64_t i0 = pos0 + static_cast<uint64_t>(lane); const uint32_t c0 = i0 < n ? rsc_code(static_cast<unsigned char>(chars[i0])) : 4u; lo0 = __ballot(c0 & 1u); hi0 = __ballot(c0 & 2u); bad0 = __ballot(c0 >> 2); }
        for (uint64_t t = pos0; t < pos_end; t += 64) {
            const uint64_t i0 = t + static_cast<uint64_t>(lane), i1 = i0 + 64;
            const uint32_t c1 = ((lane < k - 1 || t + 64 < pos_end) && i1 < n) ? rsc_code(static_cast<unsigned char>(chars[i1])) : 4u; // (the last step needs k - 1 of them)
            const uint64_t lo1 = __ballot(c1 & 1u), hi1 = __ballot(c1 & 2u), bad1 = __ballot(c1 >> 2);
            const bool ok = i0 < pos_end && (rsc_window(bad0, bad1, lane) & wmask) == 0; // (behind pos_end: the next span's; behind n: not bases)
            const uint64_t back = rsc_spread(rsc_window(lo0, lo1, lane) & wmask) | (rsc_spread(rsc_window(hi0, hi1, lane) & wmask) << 1);
            const uint64_t rc = ~back & kmask, fw = rtk_revcomp(rc, k), can = fw <= rc ? fw : rc;
            bool hit = false;
            if (ok) {
                uint64_t s = rsc_slot(can, slots);
                for (uint64_t tries = 0; tries < slots; ++tries) { const uint64_t key = T[s]; if (key == can) { hit = true; break; } if (key == RTK_RESCUE_EMPTY) break; s = s + 1 == slots ? 0 : s + 1; }
            }
            uint64_t okb = __ballot(ok ? 1 : 0), hitb = __ballot(hit ? 1 : 0);
            while (next < t + 64) { // a boundary inside this step: the positions below it are piece p's, the rest go on
                const uint64_t below = (1ull << (next - t)) - 1ull; // (t < next: p is the piece of position t)
                cw += static_cast<uint32_t>(__popcll(okb & below)); cf += static_cast<uint32_t>(__popcll(hitb & below)); okb &= ~below; hitb &= ~below;
                qv_flush(lane, p, cw, cf, windows, found); tot_w += cw; tot_f += cf; cw = 0; cf = 0;
                ++p; next = p + 1u < n_pieces ? starts[p + 1u] : ~0ull;
            }
            cw += static_cast<uint32_t>(__popcll(okb)); cf += static_cast<uint32_t>(__popcll(hitb));
            lo0 = lo1; hi0 = hi1; bad0 = bad1;
        }
        qv_flush(lane, p, cw, cf, windows, found); tot_w += cw; tot_f += cf;
    }
    if (lane < 2 && (tot_w | tot_f)) atomicAdd(totals + lane, static_cast<unsigned long long>(lane == 0 ? tot_w : tot_f));
}

struct Qv { static const char* dev() { return "hipMalloc (qv)"; } static const char* pin() { return "hipHostMalloc (qv)"; } };
template <class T> using QvDev = DevArr<T, Qv>;
template <class T> using QvPin = PinArr<T, Qv>;

struct QvJob {
    int device = 0, k = 31;
    QvDev<uint64_t> table; QvDev<unsigned long long> totals; uint64_t slots = 0, n_solid = 0; // totals: valid windows, found
    // two chunks in flight (callers on two threads overlap the copies of one with the kernel of the other); a slot is one caller's from its copy in to its copy out
    QvDev<char> d_chars[2]; QvDev<uint64_t> d_starts[2]; QvDev<uint32_t> d_counts[2]; QvPin<char> h_chars[2]; QvPin<uint64_t> h_starts[2]; QvPin<uint32_t> h_counts[2]; // counts: windows, then found
    Stream st[2]; std::mutex m[2]; std::atomic<unsigned> next{0};
    hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; std::atomic<uint64_t> kernel_us{0}; // RTK_INDEX_TRACE: the time of k_qv alone, from events around it
    std::atomic<uint64_t> chars{0}, chunks{0}; double t_table = 0.0; StageClock clk;
    ~QvJob() { for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) if (ev[i][j]) (void)hipEventDestroy(ev[i][j]); }

    void begin(int device_, int k_, const uint64_t* solid, uint64_t n) {
        device = device_; k = k_; n_solid = n;
        totals.alloc(2); rtk_check(hipMemset(totals.p, 0, 16), "hipMemset");
        slots = 2 * n + 64; // load <= 0.5: a probe ends in its first slot more often than not
        table.alloc(slots); rtk_check(hipMemset(table.p, 0xFF, 8 * slots), "hipMemset");
        if (n) {
            QvDev<uint64_t> d_solid; d_solid.alloc(n); // released when the table holds them
            rtk_check(hipMemcpy(d_solid.p, solid, 8 * n, hipMemcpyHostToDevice), "hipMemcpy");
            launch("k_qv_insert", k_qv_insert, idx_grid(n), 0, d_solid.p, n, table.p, slots);
            rtk_check(hipDeviceSynchronize(), "k_qv_insert");
        }
        for (int i = 0; i < 2; ++i) {
            d_chars[i].alloc(RTK_RESCUE_CHUNK); d_starts[i].alloc(RTK_RESCUE_READS); d_counts[i].alloc(2 * RTK_RESCUE_READS);
            h_chars[i].alloc(RTK_RESCUE_CHUNK); h_starts[i].alloc(RTK_RESCUE_READS); h_counts[i].alloc(2 * RTK_RESCUE_READS);
            st[i].create();
            if (clk.trace) for (int j = 0; j < 2; ++j) rtk_check(hipEventCreate(&ev[i][j]), "hipEventCreate");
        }
        t_table = clk.since();
        if (clk.trace) fprintf(stderr, "rtk_qv_begin: %llu k-mers, table of %llu slots in %.2f s\n", static_cast<unsigned long long>(n), static_cast<unsigned long long>(slots), t_table);
    }
    void chunk(const char* text, uint64_t n_chars, const uint64_t* starts, uint32_t n_pieces, uint32_t* windows, uint32_t* found) {
        const int sl = static_cast<int>(next.fetch_add(1) & 1u);
        std::lock_guard<std::mutex> lk(m[sl]);
        memcpy(h_chars[sl].p, text, n_chars); memcpy(h_starts[sl].p, starts, 8ull * n_pieces);
        rtk_check(hipMemcpyAsync(d_chars[sl].p, h_chars[sl].p, n_chars, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_starts[sl].p, h_starts[sl].p, 8ull * n_pieces, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemsetAsync(d_counts[sl].p, 0, 8ull * n_pieces, st[sl]), "hipMemsetAsync"); // windows[0 .. n_pieces), found[0 .. n_pieces)
        const uint64_t n_spans = (n_chars + RTK_QV_SPAN - 1) / RTK_QV_SPAN;
        if (n_spans) {
            const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((n_spans + 3) / 4, 2048)); // 4 waves per block, one span per wave and round
            if (clk.trace) rtk_check(hipEventRecord(ev[sl][0], st[sl]), "hipEventRecord");
            launch("k_qv", k_qv, dim3(blocks), st[sl], d_chars[sl].p, n_chars, d_starts[sl].p, n_pieces, k, table.p, slots, d_counts[sl].p, d_counts[sl].p + n_pieces, totals.p);
            if (clk.trace) rtk_check(hipEventRecord(ev[sl][1], st[sl]), "hipEventRecord");
        }
        rtk_check(hipMemcpyAsync(h_counts[sl].p, d_counts[sl].p, 8ull * n_pieces, hipMemcpyDeviceToHost, st[sl]), "hipMemcpyAsync");
        rtk_check(hipStreamSynchronize(st[sl]), "k_qv");
        if (clk.trace && n_spans) { float ms = 0.f; rtk_check(hipEventElapsedTime(&ms, ev[sl][0], ev[sl][1]), "hipEventElapsedTime"); kernel_us += static_cast<uint64_t>(ms * 1000.f); }
        memcpy(windows, h_counts[sl].p, 4ull * n_pieces); memcpy(found, h_counts[sl].p + n_pieces, 4ull * n_pieces);
        chars += n_chars; ++chunks;
    }
    void end(uint64_t* n_windows, uint64_t* n_found) {
        rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        unsigned long long c[2] = {0, 0}; rtk_check(hipMemcpy(c, totals.p, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_windows = c[0]; *n_found = c[1];
        if (clk.trace) fprintf(stderr, "rtk_qv: %llu characters in %llu chunks, %llu windows, %llu found; table %.2f s, k_qv %.6f s, all %.2f s\n", static_cast<unsigned long long>(chars.load()),
                               static_cast<unsigned long long>(chunks.load()), c[0], c[1], t_table, 1e-6 * static_cast<double>(kernel_us.load()), clk.since());
    }
};

} // namespace

extern "C" uint32_t rtk_qv_span(void) { return RTK_QV_SPAN; }

extern "C" int rtk_qv_begin(int device, int k, const uint64_t* solid, uint64_t n_solid, void** job_out) {
    if (!job_out || (!solid && n_solid)) return rtk_fail(RTK_ERR_ARG, "rtk_qv_begin: null argument");
    if (k < 3 || k > 31 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_qv_begin: odd k <= 31 only (one-word k-mers)");
    if (const int rc = check_device("rtk_qv_begin", device)) return rc;
    *job_out = nullptr;
    for (uint64_t i = 1; i < n_solid; ++i) if (solid[i - 1] >= solid[i]) return rtk_fail(RTK_ERR_ARG, "rtk_qv_begin: the k-mers are not sorted and distinct");
    if (n_solid && (solid[n_solid - 1] >> (2 * k))) return rtk_fail(RTK_ERR_ARG, "rtk_qv_begin: a k-mer has more than 2 k bits");
    return entry("rtk_qv_begin", device, [&]() { std::unique_ptr<QvJob> J(new QvJob()); J->begin(device, k, solid, n_solid); *job_out = J.release(); return RTK_OK; });
}

extern "C" int rtk_qv_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_pieces, uint32_t* windows, uint32_t* found) {
    QvJob* J = static_cast<QvJob*>(job);
    if (!J || !chars || !starts || !windows || !found) return rtk_fail(RTK_ERR_ARG, "rtk_qv_chunk: null argument");
    if (n_pieces == 0) return RTK_OK;
    if (n_chars > RTK_RESCUE_CHUNK || n_pieces > RTK_RESCUE_READS) return rtk_fail(RTK_ERR_ARG, "rtk_qv_chunk: chunk larger than 64 MB of characters / 4 M pieces");
    if (starts[0] != 0) return rtk_fail(RTK_ERR_ARG, "rtk_qv_chunk: the first piece must start at 0");
    for (uint32_t p = 1; p < n_pieces; ++p) if (starts[p] > n_chars || starts[p] < starts[p - 1]) return rtk_fail(RTK_ERR_ARG, "rtk_qv_chunk: piece starts must ascend and lie inside the chunk");
    return entry("rtk_qv_chunk", J->device, [&]() { J->chunk(chars, n_chars, starts, n_pieces, windows, found); return RTK_OK; });
}

extern "C" int rtk_qv_end(void* job, uint64_t* n_windows, uint64_t* n_found) {
    std::unique_ptr<QvJob> J(static_cast<QvJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_qv_end: null job");
    if (!n_windows || !n_found) return RTK_OK; // (abandoned job: released)
    *n_windows = 0; *n_found = 0;
    return entry("rtk_qv_end", J->device, [&]() { J->end(n_windows, n_found); return RTK_OK; });
}
