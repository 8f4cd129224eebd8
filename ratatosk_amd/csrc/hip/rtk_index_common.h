// What the stages of the index build's device side (rtk_index.hip and its rtk_index_*.h; rtk_rescue.hip) share: owning buffers, streams and host results, the
// rocPRIM size-query-then-run pattern, the launch and its check, one-word read-backs, the entries' checks and try/catch, and the k-mer key helpers.
#ifndef RTK_INDEX_COMMON_H
#define RTK_INDEX_COMMON_H
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <string>
#include <hip/hip_runtime.h>
#include "../../../include/ratatosk_hip.h"
#include "rtk_mem.h"
#include "rtk_types.h"
int rtk_fail(int code, const std::string& msg); // (rtk_device.hip)

namespace {
#define RTK_IDX_SENTINEL 0xFFFFFFFFFFFFFFFFull

// ------------------------------------------------------------------------------------------------ k-mer keys
typedef unsigned __int128 km2_t; // two-word k-mer (rocprim::uint128_t: radix-sortable)
__device__ __forceinline__ uint64_t idx_revcomp(uint64_t x, int k) { return rtk_revcomp(x, k); }
__device__ __forceinline__ uint64_t idx_hash(uint64_t x) { return rtk_hash64(x); }
__device__ __forceinline__ RtkKm idx_words(km2_t x) { RtkKm r; r.hi = static_cast<uint64_t>(x >> 64); r.lo = static_cast<uint64_t>(x); return r; }
__device__ __forceinline__ km2_t idx_km2(const RtkKm& x) { return (static_cast<km2_t>(x.hi) << 64) | static_cast<km2_t>(x.lo); }
__device__ __forceinline__ km2_t idx_revcomp(km2_t x, int k) { return idx_km2(rtk_km_revcomp(idx_words(x), k)); }
__device__ __forceinline__ uint64_t idx_hash(km2_t x) { return rtk_km_hash(idx_words(x)); } // (the hash of the wide k-mer table of rtk_graph_tables)
template <class KM> __device__ __forceinline__ KM idx_kmask(int k) { return (static_cast<KM>(1) << (2 * k)) - static_cast<KM>(1); }

// code of base c (A/a 0, C/c 1, G/g 2, T/t 3) or 4
__device__ __forceinline__ uint32_t idx_code(unsigned char c) {
    const unsigned char u = c & 0xDF; // upper case
    return u == 'A' ? 0u : (u == 'C' ? 1u : (u == 'G' ? 2u : (u == 'T' ? 3u : 4u)));
}

struct Iota32 { __device__ uint32_t operator()(uint64_t i) const { return static_cast<uint32_t>(i); } }; // (the payload of the sorts that give an order)

// f(KM()) with the key type of k: uint64_t (k <= 31) or km2_t (33 <= k <= 63)
template <class F> auto by_key_type(int k, F f) -> decltype(f(uint64_t())) { return k <= 31 ? f(uint64_t()) : f(km2_t()); }

// ------------------------------------------------------------------------------------------------ owners (none of them is copied)
struct Owner { Owner() {} Owner(const Owner&) = delete; Owner& operator=(const Owner&) = delete; };
struct IndexBuild { static const char* dev() { return "hipMalloc (index build)"; } static const char* pin() { return "hipHostMalloc (index build)"; } }; // a stage's tag names it in the allocation errors
// n elements of device memory (0 elements: 8 bytes, so that p is never null after alloc); adopt: memory from hipMalloc elsewhere
template <class T, class Tag = IndexBuild> struct DevArr : Owner {
    T* p = nullptr;
    ~DevArr() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    void alloc(uint64_t n) { release(); const uint64_t bytes = sizeof(T) * n; void* q = nullptr; rtk_check(hipMalloc(&q, bytes ? bytes : 8), Tag::dev()); p = static_cast<T*>(q); }
    void adopt(void* q) { release(); p = static_cast<T*>(q); }
};
// n elements of pinned host memory
template <class T, class Tag = IndexBuild> struct PinArr : Owner {
    T* p = nullptr;
    ~PinArr() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    void alloc(uint64_t n) { release(); void* q = nullptr; rtk_check(hipHostMalloc(&q, sizeof(T) * n, hipHostMallocDefault), Tag::pin()); p = static_cast<T*>(q); }
};
struct Stream : Owner {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    void create() { rtk_check(hipStreamCreate(&s), "hipStreamCreate"); }
    operator hipStream_t() const { return s; }
};
// a result for the caller (freed there with rtk_free): the entry's own until release()
template <class T> struct HostOut : Owner {
    T* p = nullptr;
    ~HostOut() { free(p); }
    bool alloc(uint64_t n) { free(p); p = static_cast<T*>(malloc(sizeof(T) * (n ? n : 1))); return p != nullptr; }
    T* release() { T* q = p; p = nullptr; return q; }
};

// ------------------------------------------------------------------------------------------------ rocPRIM, launches, read-backs
// A rocPRIM primitive is given once, as call(void* tmp, size_t& bytes) -> hipError_t: asked for the size of its temporary, `tmp` made that large, run.
template <class Call> size_t prim_bytes(const char* what, Call call) { size_t bytes = 0; rtk_check(call(nullptr, bytes), what); return bytes; }
template <class Call> void prim(void* tmp, size_t bytes, const char* what, Call call) { rtk_check(call(tmp, bytes), what); } // (a temporary sized beforehand with prim_bytes)
template <class Tag, class Call> void prim(DevArr<char, Tag>& tmp, const char* what, Call call) { const size_t bytes = prim_bytes(what, call); tmp.alloc(bytes); prim(tmp.p, bytes, what, call); }

// blocks of 256 lanes for `items` items, at least one and at most `cap` (the kernels stride over the rest)
inline dim3 idx_grid(uint64_t items, uint64_t cap = 65536) { const uint64_t b = (items + 255) / 256; return dim3(static_cast<unsigned>(b < 1 ? 1 : (b > cap ? cap : b))); }

// kernel<<<grid, 256, 0, stream>>>(args...), the arguments converted to the kernel's parameter types; a failed launch is reported as "kernel launch (name)"
template <class... P, class... A> void launch(const char* name, void (*kernel)(P...), dim3 grid, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, static_cast<P>(args)...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rtk_check(e, ("kernel launch (" + std::string(name) + ")").c_str());
}

// one value from device memory; with `synced`, after the device has gone idle (an error of the work before it is reported under that name)
template <class T> T read_word(const T* dev_ptr, const char* synced = nullptr) {
    if (synced) rtk_check(hipDeviceSynchronize(), synced);
    T v; rtk_check(hipMemcpy(&v, dev_ptr, sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
    return v;
}

// ------------------------------------------------------------------------------------------------ entries
// body() on `device`; what it throws becomes the entry's device error
template <class Body> int entry(const char* name, int device, Body body) {
    try { rtk_check(hipSetDevice(device), "hipSetDevice"); return body(); }
    catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string(name) + ": " + e.what()); }
}
inline int check_device(const char* name, int device) {
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, std::string(name) + ": no such HIP device (no CPU fallback)");
    return RTK_OK;
}
inline int check_k_and_device(const char* name, int k, int device) {
    if (k < 3 || k > 63 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, std::string(name) + ": odd k <= 63 only");
    return check_device(name, device);
}
// events of a caller (the stage entries): ascending, distinct, unitigs < n_unitigs. *n_ids (may be null): largest id + 1
inline int check_host_events(const char* name, const uint64_t* ev, uint64_t n, uint32_t n_unitigs, uint64_t* n_ids) {
    uint64_t ids = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (i && ev[i] <= ev[i - 1]) return rtk_fail(RTK_ERR_ARG, std::string(name) + ": the events are not ascending and distinct");
        if ((ev[i] >> 32) >= n_unitigs) return rtk_fail(RTK_ERR_ARG, std::string(name) + ": an event names a unitig >= n_unitigs");
        ids = std::max<uint64_t>(ids, (ev[i] & 0xFFFFFFFFull) + 1);
    }
    if (n_ids) *n_ids = ids;
    return RTK_OK;
}

// the stage's RTK_INDEX_TRACE switch and its clock
struct StageClock {
    const bool trace; const std::chrono::steady_clock::time_point t0;
    StageClock() : trace(rtk_knob_index_trace()), t0(std::chrono::steady_clock::now()) {}
    double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
} // namespace
#endif
