// The tools' way to the device: libratatosk_hip.so next to the executable's directory (BIN/../libratatosk_hip.so), loaded on request (--gpu) so
// that the plain routes need neither the library nor a GPU. Entry points by name, with the types of include/ratatosk_hip.h restated here (the
// tools do not link the library).
#ifndef RTK_COMMON_HIP_LIB_HPP
#define RTK_COMMON_HIP_LIB_HPP

#include <dlfcn.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <string>

namespace rtk {

struct HipLib {
    typedef const char* (*err_fn)(void);
    typedef void (*free_fn)(void*);
    typedef int (*count_fn)(int, int, const char* const*, int, uint32_t, int, uint64_t**, uint64_t*);                                       // rtk_index_count_kmers
    typedef int (*unitigs_fn)(int, int, const uint64_t*, uint64_t, char**, uint64_t**, uint64_t**, uint64_t*, uint64_t**, uint64_t*);        // rtk_index_unitigs
    typedef int (*col_begin_fn)(int, int, const char*, const uint64_t*, uint64_t, void**);                                                   // rtk_index_colour_begin
    typedef int (*col_chunk_fn)(void*, const char*, uint64_t, const uint64_t*, const uint32_t*, uint32_t);                                   // rtk_index_colour_chunk
    typedef int (*col_chunk_q_fn)(void*, const char*, const unsigned char*, unsigned char, uint64_t, const uint64_t*, const uint32_t*, uint32_t);     // rtk_index_colour_chunk_q
    typedef int (*col_end_fn)(void*, uint64_t**, uint64_t*, uint64_t**);                                                                     // rtk_index_colour_end
    typedef int (*col_cov_fn)(void*, uint64_t**);                                                                                            // rtk_index_colour_cov
    typedef int (*col_end_sub_fn)(void*, const uint8_t*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, double, uint64_t, uint64_t**, uint64_t*, uint64_t*, uint64_t*, uint64_t*); // rtk_index_colour_end_subsampled
    typedef int (*col_merge_fn)(void*, uint64_t*, uint64_t*, uint64_t*, uint64_t*);                                                          // rtk_index_colour_merge
    typedef int (*col_merge_classes_fn)(void*, uint64_t*, uint64_t*);                                                                        // rtk_index_colour_merge_classes
    typedef int (*snp_cand_fn)(int, int, const char*, const uint64_t*, uint64_t, const uint8_t*, uint32_t, uint64_t**, uint64_t*);                          // rtk_index_snp_candidates
    typedef int (*pair_ids_fn)(int, const uint64_t*, uint64_t, uint32_t*, uint64_t*);                                                        // rtk_index_pair_ids
    typedef int (*cover_begin_fn)(int, int, const char*, const uint64_t*, uint64_t, const uint8_t*, void**);                                 // rtk_index_cover_begin
    typedef int (*cover_chunk_fn)(void*, const char*, uint64_t, const uint64_t*, const uint32_t*, const uint64_t*, uint32_t);                // rtk_index_cover_chunk
    typedef int (*cover_end_fn)(void*, uint64_t**, uint64_t*);                                                                               // rtk_index_cover_end
    typedef int (*rescue_begin_fn)(int, int, const uint64_t*, uint64_t, const uint64_t*, uint64_t, uint32_t, void**);                        // rtk_rescue_begin
    typedef int (*rescue_chunk_fn)(void*, const char*, uint64_t, const uint64_t*, uint32_t, unsigned char*);                                 // rtk_rescue_chunk
    typedef int (*rescue_end_fn)(void*, uint64_t*, uint64_t*);                                                                               // rtk_rescue_end
    typedef int (*qv_begin_fn)(int, int, const uint64_t*, uint64_t, void**);                                                                 // rtk_qv_begin
    typedef int (*qv_chunk_fn)(void*, const char*, uint64_t, const uint64_t*, uint32_t, uint32_t*, uint32_t*);                               // rtk_qv_chunk
    typedef int (*qv_end_fn)(void*, uint64_t*, uint64_t*);                                                                                   // rtk_qv_end
    typedef int (*identity_begin_fn)(int, const char*, uint64_t, const uint64_t*, uint32_t, uint32_t, void**);                               // rtk_identity_begin
    typedef int (*identity_chunk_fn)(void*, const char*, uint64_t, const uint64_t*, uint32_t, const uint32_t*, const uint64_t*, const uint32_t*, const unsigned char*, int32_t*); // rtk_identity_chunk
    typedef int (*identity_end_fn)(void*, uint64_t*, uint64_t*);                                                                             // rtk_identity_end

    std::string path = "libratatosk_hip.so";
    void* handle = nullptr;
    err_fn last_error = nullptr; free_fn free = nullptr; count_fn count_kmers = nullptr; // what both tools need

    // false, with "TOOL: --gpu: cannot load PATH (why)" on stderr, if the library does not load
    bool open(const char* tool) {
        char exe[4096]; const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
        if (n > 0) { exe[n] = 0; std::string d(exe); d = d.substr(0, d.rfind('/')); path = d + "/../libratatosk_hip.so"; }
        handle = dlopen(path.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (!handle) { fprintf(stderr, "%s: --gpu: cannot load %s (%s)\n", tool, path.c_str(), dlerror()); return false; }
        get(last_error, "rtk_last_error"); get(free, "rtk_free"); get(count_kmers, "rtk_index_count_kmers");
        return true;
    }
    template <class Fn> bool get(Fn& fn, const char* name) const { fn = reinterpret_cast<Fn>(dlsym(handle, name)); return fn != nullptr; } // (a missing one stays null)
};

} // namespace rtk

#endif
