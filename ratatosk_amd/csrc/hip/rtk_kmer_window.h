// The bit-plane k-mer window of the kernels that test every start position of a text against a table of one-word canonical k-mers in HBM (k_rescue of
// rtk_rescue.hip, k_qv of rtk_qv.hip): 64 lanes load 64 consecutive characters, three ballots turn them into bit planes (low bit, high bit, not A/C/G/T), and a
// lane's window is k bits of each plane from its own position on -- no loop over the k characters, no branch. The planes hold the first base in the LOWEST bit.
#ifndef RTK_KMER_WINDOW_H
#define RTK_KMER_WINDOW_H
#include "rtk_index_common.h"

namespace {

// the table (open addressing, 8-byte keys, load <= 0.5) and the chunks of text that both stages take
#define RTK_RESCUE_EMPTY 0xFFFFFFFFFFFFFFFFull // (a canonical k-mer of k <= 31 has at most 62 bits)
#define RTK_RESCUE_CHUNK (64ull << 20)         // characters per rtk_rescue_chunk / rtk_qv_chunk call, as rtk_index_colour_chunk
#define RTK_RESCUE_READS (RTK_RESCUE_CHUNK / 16)

// code of base c (A/a 0, C/c 1, G/g 2, T/t 3) or 4: the upper-casing of the reads happens here
__device__ __forceinline__ uint32_t rsc_code(unsigned char c) {
    const unsigned char u = c & 0xDF;
    return u == 'A' ? 0u : (u == 'C' ? 1u : (u == 'G' ? 2u : (u == 'T' ? 3u : 4u)));
}
// bit j of x (j < 32) -> bit 2 j
__device__ __forceinline__ uint64_t rsc_spread(uint64_t x) {
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull; x = (x | (x << 8)) & 0x00FF00FF00FF00FFull; x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull; return (x | (x << 1)) & 0x5555555555555555ull;
}
// bits [lane, lane + 64) of the 128-bit plane {p1, p0}
__device__ __forceinline__ uint64_t rsc_window(uint64_t p0, uint64_t p1, int lane) { return (p0 >> lane) | ((p1 << 1) << (63 - lane)); }
__device__ __forceinline__ uint64_t rsc_slot(uint64_t can, uint64_t slots) { return __umul64hi(rtk_hash64(can), slots); }

} // namespace
#endif
