// soccer_comm.hip — soccer_comm_*: the RCCL wrapper.  Host code only (see soccer_handle.hpp).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cstring>
#include <mutex>
#include <string>

#include "soccer_handle.hpp"

// RCCL over xGMI: the job's only exchange (BASELINE configs[3]: gather of per-lane episode returns).
// librccl is resolved at run time — a process that never calls soccer_comm_* never loads it — first among the symbols
// already in the process (a host that brought its own copy), then as librccl.so.1 next to the HIP runtime.
struct IdByValue { char internal[SOCCER_COMM_ID_BYTES]; };      // ncclUniqueId: passed BY VALUE to ncclCommInitRank (rccl.h:43, :220)
namespace {
struct Rccl {
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, IdByValue, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok = false; std::string why;
};
}  // namespace

static Rccl& rccl() {
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = nullptr;
        if (!dlsym(RTLD_DEFAULT, "ncclGetUniqueId")) {
            for (const char* name : {"librccl.so.1", "librccl.so"}) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (lib) break; }
            if (!lib) { const char* e = dlerror(); R.why = std::string("librccl not found: ") + (e ? e : "?"); return; }
        }
        auto sym = [&](const char* n) -> void* { void* p = lib ? dlsym(lib, n) : dlsym(RTLD_DEFAULT, n); if (!p) R.why = std::string("librccl lacks ") + n; return p; };
        R.GetUniqueId = reinterpret_cast<decltype(R.GetUniqueId)>(sym("ncclGetUniqueId"));
        R.CommInitRank = reinterpret_cast<decltype(R.CommInitRank)>(sym("ncclCommInitRank"));
        R.CommDestroy = reinterpret_cast<decltype(R.CommDestroy)>(sym("ncclCommDestroy"));
        R.AllGather = reinterpret_cast<decltype(R.AllGather)>(sym("ncclAllGather"));
        R.AllReduce = reinterpret_cast<decltype(R.AllReduce)>(sym("ncclAllReduce"));
        R.GetErrorString = reinterpret_cast<decltype(R.GetErrorString)>(sym("ncclGetErrorString"));
        R.ok = R.GetUniqueId && R.CommInitRank && R.CommDestroy && R.AllGather && R.AllReduce && R.GetErrorString;
    });
    return R;
}
#define RCCL_TRY(h, expr)                                                                        \
    do {                                                                                         \
        const int r_ = (expr);                                                                   \
        if (r_ != 0) return fail((h), SOCCER_E_HIP, "%s failed: %s", #expr, rccl().GetErrorString(r_)); \
    } while (0)

void comm_release(soccer_handle* h) {
    if (h && h->comm) { if (rccl().ok) (void)rccl().CommDestroy(h->comm); h->comm = nullptr; h->comm_world = 0; }
}

extern "C" int soccer_comm_unique_id(uint8_t id[SOCCER_COMM_ID_BYTES]) {
    if (!id) return fail(nullptr, SOCCER_E_INVALID, "id is NULL");
    if (!rccl().ok) return fail(nullptr, SOCCER_E_HIP, "%s", rccl().why.c_str());
    static_assert(SOCCER_COMM_ID_BYTES == 128, "ncclUniqueId is 128 bytes (rccl.h: NCCL_UNIQUE_ID_BYTES)");
    RCCL_TRY(nullptr, rccl().GetUniqueId(id));
    return SOCCER_OK;
}

extern "C" int soccer_comm_init(soccer_handle* h, int32_t world, int32_t rank, const uint8_t id[SOCCER_COMM_ID_BYTES]) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_comm_init during graph capture");
    if (world < 1 || rank < 0 || rank >= world || !id) return fail(h, SOCCER_E_INVALID, "soccer_comm_init: need 0 <= rank < world and the unique id of rank 0");
    if (h->comm) return fail(h, SOCCER_E_STATE, "soccer_comm_init: this handle already has a communicator");
    if (!rccl().ok) return fail(h, SOCCER_E_HIP, "%s", rccl().why.c_str());
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->d_comm_scratch) if (int rc = h->bufs.alloc(h, 64 / sizeof(unsigned long long), &h->d_comm_scratch)) return rc;
    IdByValue v; std::memcpy(v.internal, id, sizeof v.internal);
    RCCL_TRY(h, rccl().CommInitRank(&h->comm, world, v, rank));
    h->comm_world = world; h->comm_rank = rank;
    return SOCCER_OK;
}

extern "C" int soccer_comm_destroy(soccer_handle* h) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    comm_release(h);
    return SOCCER_OK;
}

extern "C" int soccer_comm_all_gather(soccer_handle* h, const void* send, void* recv, uint64_t bytes_per_rank) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!h->comm) return fail(h, SOCCER_E_STATE, "soccer_comm_all_gather: no communicator (soccer_comm_init)");
    if (h->capturing) return fail(h, SOCCER_E_STATE, "soccer_comm_all_gather during graph capture");
    if (!send || !recv) return fail(h, SOCCER_E_INVALID, "soccer_comm_all_gather: send/recv is NULL");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    RCCL_TRY(h, rccl().AllGather(send, recv, (size_t)bytes_per_rank, /*ncclInt8*/ 0, h->comm, h->stream));
    return SOCCER_OK;
}

// small host-value reductions through the handle's 64-byte device scratch: up to 8 values, SUM of uint64 or MAX of float64.
// Synchronises (the result is returned to the host) — which also makes it the job's barrier.
static int comm_reduce_small(soccer_handle* h, void* values, int32_t count, bool f64_max, const char* what) {
    if (!h) return fail(nullptr, SOCCER_E_INVALID, "handle is NULL");
    if (!h->comm) return fail(h, SOCCER_E_STATE, "%s: no communicator (soccer_comm_init)", what);
    if (h->capturing) return fail(h, SOCCER_E_STATE, "%s during graph capture", what);
    if (!values || count < 1 || count > 8) return fail(h, SOCCER_E_INVALID, "%s: 1..8 values", what);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(h->d_comm_scratch, values, 8 * (size_t)count, hipMemcpyHostToDevice, h->stream));
    RCCL_TRY(h, rccl().AllReduce(h->d_comm_scratch, h->d_comm_scratch, (size_t)count, f64_max ? /*ncclFloat64*/ 8 : /*ncclUint64*/ 5,
                                 f64_max ? /*ncclMax*/ 2 : /*ncclSum*/ 0, h->comm, h->stream));
    HIP_TRY(h, hipMemcpyAsync(values, h->d_comm_scratch, 8 * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return SOCCER_OK;
}
extern "C" int soccer_comm_sum_u64(soccer_handle* h, uint64_t* values, int32_t count) { return comm_reduce_small(h, values, count, false, "soccer_comm_sum_u64"); }
extern "C" int soccer_comm_max_f64(soccer_handle* h, double* values, int32_t count) { return comm_reduce_small(h, values, count, true, "soccer_comm_max_f64"); }
extern "C" int soccer_comm_barrier(soccer_handle* h) { uint64_t one = 1; return comm_reduce_small(h, &one, 1, false, "soccer_comm_barrier"); }
