// The hash of a read name for --pair-by-name (DESIGN.md section 4 [A18]): 64-bit FNV-1a over the bytes of the name, then the mixer of the k-mer tables (hash64,
// kmer.hpp; rtk_hash64 on the device) so that the top bits, which cut the hash space into passes on the device, are mixed. Two names are the same when their hashes
// are -- the contract of the reference's name_hmap, which keys by the wyhash of the name (src/Graph.cpp:1595-1608).
#ifndef RTK_COMMON_NAME_HASH_HPP
#define RTK_COMMON_NAME_HASH_HPP

#include <cstddef>
#include <cstdint>

#include "kmer.hpp"

namespace rtk {

inline uint64_t name_hash(const char* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ULL;
    for (size_t i = 0; i < n; ++i) { h ^= static_cast<unsigned char>(p[i]); h *= 0x100000001b3ULL; }
    return hash64(h);
}

} // namespace rtk

#endif
