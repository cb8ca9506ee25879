// C ABI, pooling over GPUs (bmc_comm_*, bmc_allgather): RCCL, loaded on first use
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>

#include "bmc_ctx.h"

namespace {
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t,
                              hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
// One RCCL per process: the copy already in the process (torch loads its own, same soname)
// wins; otherwise the loader's search path, then the ROCm install.  BMC_RCCL_SONAME (tests
// only) replaces the candidate list, so that a failing load can be exercised.
// The table is built ONCE, by a function-local static (C++11: thread-safe, so two host threads
// that drive two contexts cannot see it half filled); the loader's error text is taken right
// after the failing dlopen / dlsym -- dlerror() clears itself when read -- and kept.
struct RcclLoad {
    Rccl r;
    std::string err;
};
RcclLoad load_rccl() {
    RcclLoad L;
    Rccl& r = L.r;
    std::vector<std::string> names;
    if (const char* forced = std::getenv("BMC_RCCL_SONAME")) names = {forced};
    else names = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const std::string& name : names)
        if (!r.h) r.h = dlopen(name.c_str(), RTLD_NOW | RTLD_NOLOAD);
    for (const std::string& name : names)
        if (!r.h) {
            (void)dlerror();
            r.h = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL);
            if (!r.h) {
                const char* e = dlerror();
                L.err = e ? e : (name + ": dlopen failed");
            }
        }
    if (!r.h) {
        if (L.err.empty()) L.err = "librccl.so.1 not found";
        return L;
    }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.h, "ncclCommInitRank");
    r.AllGather = (decltype(r.AllGather))dlsym(r.h, "ncclAllGather");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.h, "ncclCommDestroy");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllGather || !r.CommDestroy || !r.GetErrorString) {
        r.h = nullptr;
        L.err = "RCCL symbols missing (ncclGetUniqueId / ncclCommInitRank / ncclAllGather / "
                "ncclCommDestroy / ncclGetErrorString)";
    }
    return L;
}
const RcclLoad& rccl_state() {
    static const RcclLoad L = load_rccl();
    return L;
}
const Rccl* rccl() {
    const RcclLoad& L = rccl_state();
    return L.r.h ? &L.r : nullptr;
}
#define RCCLCHK(ctx, R, expr)                                                          \
    do {                                                                               \
        ncclResult_t r__ = (expr);                                                     \
        if (r__ != ncclSuccess)                                                        \
            return fail(ctx, BMC_EHIP, std::string(#expr) + ": " + (R)->GetErrorString(r__)); \
    } while (0)
}  // namespace

extern "C" {

int bmc_comm_unique_id(char id_out[BMC_COMM_ID_BYTES]) {
    static_assert(BMC_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    if (!id_out) return BMC_EINVAL;
    const Rccl* R = rccl();
    if (!R) return BMC_EHIP;
    ncclUniqueId id;
    if (R->GetUniqueId(&id) != ncclSuccess) return BMC_EHIP;
    std::memcpy(id_out, id.internal, BMC_COMM_ID_BYTES);
    return BMC_OK;
}

int bmc_comm_destroy(bmc_ctx* c) {
    if (!c) return BMC_EINVAL;
    if (c->comm) {
        const Rccl* R = rccl();
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (R) (void)R->CommDestroy(c->comm);
        c->comm = nullptr;
        c->comm_world = c->comm_rank = 0;
    }
    return BMC_OK;
}

int bmc_comm_init(bmc_ctx* c, int32_t world, int32_t rank, const char id[BMC_COMM_ID_BYTES]) {
    if (!c) return BMC_EINVAL;
    if (!id || world < 1 || rank < 0 || rank >= world)
        return fail(c, BMC_EINVAL, "need world >= 1, 0 <= rank < world and an id");
    const Rccl* R = rccl();
    if (!R) return fail(c, BMC_EHIP, "RCCL could not be loaded: " + rccl_state().err);
    HIPCHK(c, hipSetDevice(c->device));
    bmc_comm_destroy(c);
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, BMC_COMM_ID_BYTES);
    RCCLCHK(c, R, R->CommInitRank(&c->comm, world, uid, rank));
    c->comm_world = world;
    c->comm_rank = rank;
    return BMC_OK;
}

int bmc_allgather(bmc_ctx* c, const void* d_send, void* d_recv, int64_t count_per_rank) {
    if (!c) return BMC_EINVAL;
    if (!c->comm) return fail(c, BMC_ESTATE, "bmc_comm_init must be called first");
    if (!d_send || !d_recv || count_per_rank < 0) return fail(c, BMC_EINVAL, "bad arguments");
    const Rccl* R = rccl();
    if (!R) return fail(c, BMC_EHIP, "RCCL is not loaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (count_per_rank > 0)
        RCCLCHK(c, R, R->AllGather(d_send, d_recv, (size_t)count_per_rank, ncclFloat64, c->comm,
                                   c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BMC_OK;
}

}  // extern "C"
