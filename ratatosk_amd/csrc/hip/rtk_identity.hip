// Identity of reads to their simulated truth (rtk_identity, `correct --truth-ref --truth-tsv`; DESIGN.md section 4, [A19]): the exact unit-cost NW distance of
// every read and the stretch of the reference it was drawn from. No counterpart in the reference: the project's own measure, like rtk_qv.
//   rtk_identity_begin   the reference text copied to HBM once; one work area per wave, sized by max_len, for two chunks in flight
//   rtk_identity_chunk   k_identity: persistent waves take (read, stretch) pairs off one counter, heaviest first (the order is made here, on the host, when the
//                        chunk is packed); a wave writes the stretch into its work area straight from the resident reference -- reversed and complemented on
//                        the way for strand '-' -- and calls rtk_myers_distance(NW, k = -1, bytes equal iff identical). One distance per read, nothing stored
//                        for a traceback.
//   rtk_identity_end     pairs and distance sum of the job; releases it
// The aligner is used as it is (rtk_myers.h): the one-row-block sweep up to 4096 rows, above that the banded passes -- ring or row blocks -- with their
// guess-then-settle second pass. One wave per pair; see profiles/identity.txt for what that costs at the tail of a launch.
#include <string.h>

#include <atomic>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rtk_index_common.h" // the owners and entry helpers of the index build's device side
#include "rtk_myers.h"        // the aligner, compiled for one wave per workgroup

namespace {

#define RTK_IDENTITY_CHUNK (64ull << 20) // characters per chunk call, as rtk_qv_chunk
#define RTK_IDENTITY_READS (4u << 20)    // reads per chunk call
#define RTK_IDENTITY_MAX_LEN (1u << 24)  // largest max_len a job takes: lengths are ints in the aligner, work areas grow by ~16 bytes per character

// one pair of a chunk, in the order the waves take them
struct IdPair { uint64_t q_off, t_off; uint32_t qlen, tlen, rev, out; };

__device__ __forceinline__ char id_complement(char c) { return c == 'A' ? 'T' : (c == 'T' ? 'A' : (c == 'C' ? 'G' : (c == 'G' ? 'C' : c))); }

// One wave per workgroup. pairs[0 .. n) are sorted heaviest first; a wave takes the next one off *counter until none is left. The stretch of pair p is
// ref[t_off .. t_off + tlen), written to the wave's own `truth` buffer behind its aligner work area (reversed and complemented when rev), then aligned against
// chars[q_off .. q_off + qlen). dist[out] = the distance; status |= the aligner's overflow word (a capacity of the work area was exceeded: the host sized it
// by max_len and checked every length, so this is an error of the library). totals[0] += pairs, totals[1] += distances: one atomic pair per wave.
// wave_clock (trace only, else null): wall-clock ticks at which wave w took its first pair and finished its last.
__global__ void __launch_bounds__(64) k_identity(const IdPair* __restrict__ pairs, uint32_t n, const char* __restrict__ chars, const char* __restrict__ ref, char* scratch, uint64_t stride, ScratchCfg cfg,
                                                 uint32_t* counter, int32_t* dist, uint32_t* status, unsigned long long* totals, unsigned long long* wave_clock) {
    __shared__ MyersScratch sc; // in LDS, as the aligner assumes (RTK_ASSUME_LDS)
    char* const base = scratch + static_cast<uint64_t>(blockIdx.x) * stride;
    sc = scratch_carve(base, cfg); // every lane stores the same words
    __syncthreads();
    char* const truth = base + scratch_bytes(cfg);
    const int lane = rtk_lane();
    unsigned long long n_done = 0, sum = 0;
    if (wave_clock && lane == 0) wave_clock[2 * blockIdx.x] = wall_clock64();
    for (;;) {
        uint32_t i = 0;
        if (lane == 0) i = atomicAdd(counter, 1u);
        i = rtk_u(i);
        if (i >= n) break;
        const uint64_t q_off = rtk_u(pairs[i].q_off), t_off = rtk_u(pairs[i].t_off);
        const uint32_t qlen = rtk_u(pairs[i].qlen), tlen = rtk_u(pairs[i].tlen), rev = rtk_u(pairs[i].rev), out = rtk_u(pairs[i].out);
        const char* const src = ref + t_off;
        if (rev) for (uint32_t j = static_cast<uint32_t>(lane); j < tlen; j += 64u) truth[j] = id_complement(src[tlen - 1u - j]);
        else for (uint32_t j = static_cast<uint32_t>(lane); j < tlen; j += 64u) truth[j] = src[j];
        *sc.overflow = 0;
        rtk_sync(); // the stretch is written
        const MyersResult r = rtk_myers_distance(sc, chars + q_off, static_cast<int>(qlen), truth, static_cast<int>(tlen), -1, RTK_MODE_NW, false);
        rtk_sync(); // the aligner is done with the stretch
        const uint32_t ov = *sc.overflow;
        if (lane == 0) { dist[out] = r.dist; if (ov || r.dist < 0) atomicOr(status, 1u); }
        ++n_done; sum += static_cast<unsigned long long>(r.dist < 0 ? 0 : r.dist);
    }
    if (lane == 0 && n_done) { atomicAdd(totals, n_done); atomicAdd(totals + 1, sum); }
    if (wave_clock && lane == 0) wave_clock[2 * blockIdx.x + 1] = wall_clock64();
}

struct Identity { static const char* dev() { return "hipMalloc (identity)"; } static const char* pin() { return "hipHostMalloc (identity)"; } };
template <class T> using IdDev = DevArr<T, Identity>;
template <class T> using IdPin = PinArr<T, Identity>;

// what a wave needs for pairs of up to max_len characters on either side: the aligner's words, target columns, last-column scores and the delta vectors of the
// banded pass (kept where a traceback table would be: the distance call stores no table, so that is all the room it needs there), no moves
ScratchCfg identity_cfg(uint32_t max_len) {
    ScratchCfg c; c.w_cap = (max_len + 63) / 64 + 1; c.t_cap = max_len + 64; c.r_cap = max_len + 64; c.mv_cap = 64;
    c.tb_cap_words = 4ull * c.w_cap + 64;
    return c;
}
uint64_t identity_stride(uint32_t max_len) { return scratch_bytes(identity_cfg(max_len)) + (static_cast<uint64_t>(max_len) + 64 + 255) / 256 * 256; }

// the order of the waves: m x estimated band. One row block (m <= 4096) sweeps whole columns; above that the first pass runs in the band of the aligner's guess
uint64_t identity_weight(uint32_t m, uint32_t n) {
    if (m == 0 || n == 0) return 0;
    const uint64_t band = m <= 4096 ? n : std::min<uint64_t>(n, static_cast<uint64_t>(rtk_band_guess(static_cast<int>(m), static_cast<int>(n))));
    return static_cast<uint64_t>(m) * band;
}

struct IdentityJob {
    int device = 0; uint32_t max_len = 0, n_rec = 0, waves = 0; uint64_t n_ref = 0, stride = 0; ScratchCfg cfg;
    std::vector<uint64_t> rec_off; // [n_rec + 1]
    IdDev<char> d_ref; IdDev<unsigned long long> totals;
    // two chunks in flight; a slot is one caller's from its copy in to its copy out
    IdDev<char> d_chars[2], d_scratch[2]; IdDev<IdPair> d_pairs[2]; IdDev<int32_t> d_dist[2]; IdDev<uint32_t> d_ctl[2]; IdDev<unsigned long long> d_clock[2]; // ctl: counter, status
    IdPin<char> h_chars[2]; IdPin<IdPair> h_pairs[2]; IdPin<int32_t> h_dist[2]; IdPin<uint32_t> h_ctl[2]; IdPin<unsigned long long> h_clock[2];
    uint32_t cap[2] = {0, 0}; // reads the pair and distance buffers of a slot hold: they grow with the chunks (4 M reads of 36 bytes, twice over, on both sides of the bus, is room few jobs need)
    Stream st[2]; std::mutex m[2]; std::atomic<unsigned> next{0};
    hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    std::atomic<uint64_t> kernel_us{0}, chars{0}, chunks{0}, pairs{0}, span_ticks{0}, tail_ticks{0}; StageClock clk;
    ~IdentityJob() { for (int i = 0; i < 2; ++i) for (int j = 0; j < 2; ++j) if (ev[i][j]) (void)hipEventDestroy(ev[i][j]); }

    void begin(int device_, const char* ref, uint64_t n_ref_, const uint64_t* off, uint32_t n_rec_, uint32_t max_len_) {
        device = device_; n_ref = n_ref_; n_rec = n_rec_; max_len = max_len_ ? max_len_ : 1; rec_off.assign(off, off + n_rec + 1);
        cfg = identity_cfg(max_len); stride = identity_stride(max_len); waves = static_cast<uint32_t>(rtk_knob_identity_waves());
        const uint64_t per_slot = RTK_IDENTITY_CHUNK + static_cast<uint64_t>(RTK_IDENTITY_READS) * (sizeof(IdPair) + 4);
        const uint64_t need = n_ref + 64 + 2 * (static_cast<uint64_t>(waves) * stride + per_slot);
        size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
        if (need > fr) throw std::runtime_error("the reference, the work areas of 2 x " + std::to_string(waves) + " waves for pairs of up to " + std::to_string(max_len) + " characters and the chunk buffers need " +
                                                std::to_string(need) + " bytes of device memory, " + std::to_string(fr) + " bytes are free");
        d_ref.alloc(n_ref + 64);
        if (n_ref) rtk_check(hipMemcpy(d_ref.p, ref, n_ref, hipMemcpyHostToDevice), "hipMemcpy");
        totals.alloc(2); rtk_check(hipMemset(totals.p, 0, 16), "hipMemset");
        for (int i = 0; i < 2; ++i) {
            d_chars[i].alloc(RTK_IDENTITY_CHUNK + 64); d_ctl[i].alloc(2); d_scratch[i].alloc(static_cast<uint64_t>(waves) * stride);
            h_chars[i].alloc(RTK_IDENTITY_CHUNK); h_ctl[i].alloc(2);
            st[i].create();
            if (clk.trace) { for (int j = 0; j < 2; ++j) rtk_check(hipEventCreate(&ev[i][j]), "hipEventCreate"); d_clock[i].alloc(2ull * waves); h_clock[i].alloc(2ull * waves); }
        }
        if (clk.trace) fprintf(stderr, "rtk_identity_begin: %llu reference characters in %u records, 2 x %u work areas of %llu bytes (max_len %u) in %.2f s\n", static_cast<unsigned long long>(n_ref), n_rec, waves,
                               static_cast<unsigned long long>(stride), max_len, clk.since());
    }
    // (every length and stretch has been checked by the entry)
    void chunk(const char* text, uint64_t n_chars, const uint64_t* starts, uint32_t n, const uint32_t* rec, const uint64_t* t_start, const uint32_t* t_len, const unsigned char* rev, int32_t* dist) {
        std::vector<std::pair<uint64_t, uint32_t> > order(n); // (weight, read), heaviest first; equal weights in input order
        for (uint32_t i = 0; i < n; ++i) { const uint64_t e = i + 1 < n ? starts[i + 1] : n_chars; order[i] = std::make_pair(identity_weight(static_cast<uint32_t>(e - starts[i] - 1), t_len[i]), i); }
        std::sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
        const int sl = static_cast<int>(next.fetch_add(1) & 1u);
        std::lock_guard<std::mutex> lk(m[sl]);
        if (n > cap[sl]) { const uint32_t c = std::min<uint64_t>(RTK_IDENTITY_READS, std::max<uint64_t>(n, std::max<uint64_t>(2ull * cap[sl], 65536))); d_pairs[sl].alloc(c); d_dist[sl].alloc(c); h_pairs[sl].alloc(c); h_dist[sl].alloc(c); cap[sl] = c; }
        memcpy(h_chars[sl].p, text, n_chars);
        for (uint32_t x = 0; x < n; ++x) {
            const uint32_t i = order[x].second; const uint64_t e = i + 1 < n ? starts[i + 1] : n_chars;
            IdPair& p = h_pairs[sl].p[x]; p.q_off = starts[i]; p.qlen = static_cast<uint32_t>(e - starts[i] - 1); p.t_off = rec_off[rec[i]] + t_start[i]; p.tlen = t_len[i]; p.rev = rev[i] ? 1u : 0u; p.out = i;
        }
        const unsigned grid = std::min<uint32_t>(n, waves);
        rtk_check(hipMemcpyAsync(d_chars[sl].p, h_chars[sl].p, n_chars, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_pairs[sl].p, h_pairs[sl].p, sizeof(IdPair) * n, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemsetAsync(d_ctl[sl].p, 0, 8, st[sl]), "hipMemsetAsync");
        if (clk.trace) rtk_check(hipEventRecord(ev[sl][0], st[sl]), "hipEventRecord");
        rtk_launch(k_identity, static_cast<int>(grid), st[sl], static_cast<const IdPair*>(d_pairs[sl].p), n, static_cast<const char*>(d_chars[sl].p), static_cast<const char*>(d_ref.p), d_scratch[sl].p, stride, cfg,
                   d_ctl[sl].p, d_dist[sl].p, d_ctl[sl].p + 1, totals.p, clk.trace ? d_clock[sl].p : static_cast<unsigned long long*>(nullptr));
        if (clk.trace) rtk_check(hipEventRecord(ev[sl][1], st[sl]), "hipEventRecord");
        rtk_check(hipMemcpyAsync(h_dist[sl].p, d_dist[sl].p, 4ull * n, hipMemcpyDeviceToHost, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(h_ctl[sl].p, d_ctl[sl].p, 8, hipMemcpyDeviceToHost, st[sl]), "hipMemcpyAsync");
        if (clk.trace) rtk_check(hipMemcpyAsync(h_clock[sl].p, d_clock[sl].p, 16ull * grid, hipMemcpyDeviceToHost, st[sl]), "hipMemcpyAsync");
        rtk_check(hipStreamSynchronize(st[sl]), "k_identity");
        if (h_ctl[sl].p[1]) throw std::runtime_error("k_identity: a work area sized for " + std::to_string(max_len) + " characters was exceeded");
        memcpy(dist, h_dist[sl].p, 4ull * n);
        if (clk.trace) {
            float ms = 0.f; rtk_check(hipEventElapsedTime(&ms, ev[sl][0], ev[sl][1]), "hipEventElapsedTime"); kernel_us += static_cast<uint64_t>(ms * 1000.f);
            unsigned long long first = ~0ull, last = 0, before_last = 0; // the launch from its first wave's start; its end, and the end of the last wave but one
            for (unsigned w = 0; w < grid; ++w) { const unsigned long long a = h_clock[sl].p[2 * w], b = h_clock[sl].p[2 * w + 1]; first = std::min(first, a); if (b > last) { before_last = last; last = b; } else if (b > before_last) before_last = b; }
            span_ticks += last - first; if (grid > 1) tail_ticks += last - before_last;
        }
        chars += n_chars; ++chunks; pairs += n;
    }
    void end(uint64_t* n_pairs, uint64_t* sum_dist) {
        rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        unsigned long long c[2] = {0, 0}; rtk_check(hipMemcpy(c, totals.p, 16, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_pairs = c[0]; *sum_dist = c[1];
        if (clk.trace) fprintf(stderr, "rtk_identity: %llu characters in %llu chunks, %llu pairs, distance sum %llu; k_identity %.6f s, of its launches' %llu clock ticks %llu after the last wave but one had finished; all %.2f s\n",
                               static_cast<unsigned long long>(chars.load()), static_cast<unsigned long long>(chunks.load()), c[0], c[1], 1e-6 * static_cast<double>(kernel_us.load()),
                               static_cast<unsigned long long>(span_ticks.load()), static_cast<unsigned long long>(tail_ticks.load()), clk.since());
    }
};

} // namespace

extern "C" int rtk_identity_begin(int device, const char* ref, uint64_t n_ref, const uint64_t* rec_off, uint32_t n_rec, uint32_t max_len, void** job_out) {
    if (!job_out || !rec_off || (!ref && n_ref)) return rtk_fail(RTK_ERR_ARG, "rtk_identity_begin: null argument");
    *job_out = nullptr;
    if (max_len > RTK_IDENTITY_MAX_LEN) return rtk_fail(RTK_ERR_ARG, "rtk_identity_begin: max_len above " + std::to_string(RTK_IDENTITY_MAX_LEN));
    if (rec_off[0] != 0 || rec_off[n_rec] > n_ref) return rtk_fail(RTK_ERR_ARG, "rtk_identity_begin: the records must start at 0 and end inside the reference");
    for (uint32_t r = 0; r < n_rec; ++r) if (rec_off[r] > rec_off[r + 1]) return rtk_fail(RTK_ERR_ARG, "rtk_identity_begin: record offsets must ascend");
    if (const int rc = check_device("rtk_identity_begin", device)) return rc;
    return entry("rtk_identity_begin", device, [&]() { std::unique_ptr<IdentityJob> J(new IdentityJob()); J->begin(device, ref, n_ref, rec_off, n_rec, max_len); *job_out = J.release(); return RTK_OK; });
}

extern "C" int rtk_identity_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_reads, const uint32_t* rec, const uint64_t* t_start, const uint32_t* t_len,
                                  const unsigned char* rev, int32_t* dist) {
    IdentityJob* J = static_cast<IdentityJob*>(job);
    if (!J || !chars || !starts || !rec || !t_start || !t_len || !rev || !dist) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: null argument");
    if (n_reads == 0) return RTK_OK;
    if (n_chars > RTK_IDENTITY_CHUNK || n_reads > RTK_IDENTITY_READS) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: chunk larger than 64 MB of characters / 4 M reads");
    if (starts[0] != 0) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: the first read must start at 0");
    for (uint32_t i = 0; i < n_reads; ++i) { // nothing is launched for a chunk that holds one bad pair
        const uint64_t e = i + 1 < n_reads ? starts[i + 1] : n_chars;
        if (e > n_chars || e <= starts[i]) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: read starts must ascend, lie inside the chunk and leave room for the separator (read " + std::to_string(i) + ")");
        if (e - starts[i] - 1 > J->max_len || t_len[i] > J->max_len) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: read " + std::to_string(i) + " or its stretch is longer than the job's max_len " + std::to_string(J->max_len));
        if (rec[i] >= J->n_rec) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: read " + std::to_string(i) + " names record " + std::to_string(rec[i]) + " of " + std::to_string(J->n_rec));
        const uint64_t rl = J->rec_off[rec[i] + 1] - J->rec_off[rec[i]];
        if (t_start[i] > rl || t_len[i] > rl - t_start[i]) return rtk_fail(RTK_ERR_ARG, "rtk_identity_chunk: the stretch of read " + std::to_string(i) + " lies outside record " + std::to_string(rec[i]) + " (" + std::to_string(rl) + " characters)");
    }
    return entry("rtk_identity_chunk", J->device, [&]() { J->chunk(chars, n_chars, starts, n_reads, rec, t_start, t_len, rev, dist); return RTK_OK; });
}

extern "C" int rtk_identity_end(void* job, uint64_t* n_pairs, uint64_t* sum_dist) {
    std::unique_ptr<IdentityJob> J(static_cast<IdentityJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_identity_end: null job");
    if (!n_pairs || !sum_dist) return RTK_OK; // (abandoned job: released)
    *n_pairs = 0; *sum_dist = 0;
    return entry("rtk_identity_end", J->device, [&]() { J->end(n_pairs, sum_dist); return RTK_OK; });
}
