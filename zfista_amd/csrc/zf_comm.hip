// zf_comm.hip - RCCL inside the library ("context create(device id, optional RCCL
// rank/world/unique-id)"; 8e: the exchanges C1 / C2 of a sharded decision vector).
//
// A zf_comm wraps one ncclComm_t (RCCL over xGMI, one rank per GPU).  Attached to a solver
// (zf_solver_set_comm) it lets zf_solver_enqueue_init / zf_solver_enqueue_steps issue the packed
// all-gathers of a sharded step themselves, on the solver's stream, between the trial and the
// decide kernel: a multi-rank pass needs no host code per pass (round 1 drove it from a Python loop
// through torch.distributed).  The rank-ordered summation of the gathered packs stays where it was
// (zf_decide_kernel, zf_sum_parts_kernel): all ranks take bitwise-identical decisions.
//
// librccl is loaded with dlopen at the first zf_comm call - the library itself has no link-time
// dependency on it and single-GPU users never touch it.  Inside a process that already loaded
// RCCL (PyTorch does) the same soname resolves to that copy.
#include <dlfcn.h>
#include <pthread.h>

#include <mutex>
#include <new>

#include "zf_common.h"

namespace {
typedef void* nccl_comm_t;
struct nccl_unique_id {
    char internal[128];
};
struct rccl_api {
    void* handle = nullptr;
    int (*GetUniqueId)(nccl_unique_id*) = nullptr;
    int (*CommInitRank)(nccl_comm_t*, int, nccl_unique_id, int) = nullptr;
    int (*CommDestroy)(nccl_comm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, nccl_comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    // what the communicator says about itself (zf_comm_describe): optional symbols
    int (*CommCount)(nccl_comm_t, int*) = nullptr;
    int (*CommUserRank)(nccl_comm_t, int*) = nullptr;
    int (*CommCuDevice)(nccl_comm_t, int*) = nullptr;
    int (*GetVersion)(int*) = nullptr;
    char path[256] = "";
};
rccl_api g_rccl;

std::once_flag g_rccl_once;
char g_rccl_err[256] = "";

// (once per process, whatever thread gets here first: rank threads of a local group may race to it)
void rccl_load_once() {
    // ZF_RCCL_LIB names the one library to use (a pinned RCCL build; tests: a path that does not exist).  The only getenv
    // outside zf_env_read (zf_solver.hip): the library is loaded once per process, not per solver.
    const char* pinned = getenv("ZF_RCCL_LIB");
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    if (pinned && *pinned) {
        h = dlopen(pinned, RTLD_NOW | RTLD_GLOBAL);
    } else {
        for (const char* n : names) {
            h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
    }
    if (!h) {
        snprintf(g_rccl_err, sizeof(g_rccl_err), "zf_comm: cannot load librccl (%s)", dlerror());
        return;
    }
    g_rccl.GetUniqueId = (int (*)(nccl_unique_id*))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(nccl_comm_t*, int, nccl_unique_id, int))dlsym(h, "ncclCommInitRank");
    g_rccl.CommDestroy = (int (*)(nccl_comm_t))dlsym(h, "ncclCommDestroy");
    g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, nccl_comm_t, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather) {
        snprintf(g_rccl_err, sizeof(g_rccl_err), "zf_comm: librccl lacks an expected symbol");
        return;
    }
    g_rccl.CommCount = (int (*)(nccl_comm_t, int*))dlsym(h, "ncclCommCount");
    g_rccl.CommUserRank = (int (*)(nccl_comm_t, int*))dlsym(h, "ncclCommUserRank");
    g_rccl.CommCuDevice = (int (*)(nccl_comm_t, int*))dlsym(h, "ncclCommCuDevice");
    g_rccl.GetVersion = (int (*)(int*))dlsym(h, "ncclGetVersion");
    Dl_info info;
    if (dladdr((void*)g_rccl.AllGather, &info) && info.dli_fname) snprintf(g_rccl.path, sizeof(g_rccl.path), "%s", info.dli_fname);
    g_rccl.handle = h;
}
int rccl_load() {
    std::call_once(g_rccl_once, rccl_load_once);
    if (!g_rccl.handle) return zf_fail(ZF_ERR_STATE, "%s", g_rccl_err);
    return ZF_OK;
}
int rccl_check(int rc, const char* what) {
    if (rc == 0) return ZF_OK;
    return zf_fail(ZF_ERR_STATE, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
}
}  // namespace

// In-process stand-in for a communicator (tests on ONE GPU: RCCL places one rank per device): `world`
// host threads, one per emulated rank, each with its own stream.  An all-gather copies the rank's
// contribution into a shared staging buffer, meets the other threads at a host barrier (so that every
// rank's copy-in is enqueued and its event recorded), makes its stream wait for all copy-ins and copies
// the gathered block out.  Staging is double-buffered by call parity: a rank's copy-in of call k + 2
// is stream-ordered after its copy-out of k + 1, which waited for every other rank's copy-in of k + 1,
// which those ranks enqueued after their copy-out of call k.
struct zf_local_group {
    int world = 0;
    int64_t cap = 0;                  // doubles per rank and parity
    double* staging = nullptr;        // [2][world][cap]
    hipEvent_t* ev = nullptr;         // [2][world]
    pthread_barrier_t barrier;
    int failed[2] = {0, 0};           // per parity: some rank could not contribute to the call in flight
    int refs = 0;
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
};

struct zf_comm {
    nccl_comm_t comm = nullptr;
    int rank = 0, world = 1;
    zf_local_group* local = nullptr;  // non-NULL: the in-process stand-in
    unsigned calls = 0;
    int64_t gathers = 0;              // all-gathers issued on this communicator (zf_comm_describe)
};

// 128 bytes that rank 0 creates and every rank of the communicator must receive (over any host
// channel: a file, MPI, torch.distributed, a socket) before zf_comm_create
extern "C" int zf_comm_unique_id(void* id128) {
    ZF_REQUIRE(id128, "zf_comm_unique_id: null argument");
    int rc = rccl_load();
    if (rc) return rc;
    return rccl_check(g_rccl.GetUniqueId(static_cast<nccl_unique_id*>(id128)), "ncclGetUniqueId");
}

// collective over the `world` ranks: every rank calls it with the same id, its own rank, and with
// its GPU current (zf_set_device / hipSetDevice)
extern "C" int zf_comm_create(zf_comm** out, int32_t rank, int32_t world, const void* id128) {
    ZF_REQUIRE(out && id128 && world >= 1 && rank >= 0 && rank < world, "zf_comm_create: bad argument");
    int rc = rccl_load();
    if (rc) return rc;
    zf_comm* c = new (std::nothrow) zf_comm();
    if (!c) return zf_fail(ZF_ERR_ARG, "zf_comm_create: out of host memory");
    nccl_unique_id id;
    memcpy(&id, id128, sizeof(id));
    rc = rccl_check(g_rccl.CommInitRank(&c->comm, world, id, rank), "ncclCommInitRank");
    if (rc) {
        delete c;
        return rc;
    }
    c->rank = rank;
    c->world = world;
    *out = c;
    return ZF_OK;
}

// `world` communicators of one in-process group (see zf_local_group): out[r] belongs to the host
// thread that plays rank r.  cap_doubles bounds the count of any all-gather on them.
extern "C" int zf_comm_create_local_group(zf_comm** out, int32_t world, int64_t cap_doubles) {
    ZF_REQUIRE(out && world >= 1 && cap_doubles >= 1, "zf_comm_create_local_group: bad argument");
    zf_local_group* g = new (std::nothrow) zf_local_group();
    if (!g) return zf_fail(ZF_ERR_ARG, "zf_comm_create_local_group: out of host memory");
    g->world = world;
    g->cap = cap_doubles;
    g->refs = world;
    // everything is released again on any failure below: nothing of a half-built group is handed out
    int made_ev = 0, made_c = 0;
    bool barrier_ok = false;
    hipError_t e = hipMalloc(&g->staging, sizeof(double) * 2 * world * cap_doubles);
    if (e == hipSuccess) {
        g->ev = new (std::nothrow) hipEvent_t[2 * world];
        if (!g->ev) e = hipErrorOutOfMemory;
    }
    for (; e == hipSuccess && made_ev < 2 * world; ++made_ev)
        e = hipEventCreateWithFlags(&g->ev[made_ev], hipEventDisableTiming);
    if (e != hipSuccess) made_ev = made_ev > 0 ? made_ev - 1 : 0;   // (the failing create made none)
    if (e == hipSuccess) barrier_ok = pthread_barrier_init(&g->barrier, nullptr, (unsigned)world) == 0;
    if (e == hipSuccess && barrier_ok) {
        for (; made_c < world; ++made_c) {
            zf_comm* c = new (std::nothrow) zf_comm();
            if (!c) break;
            c->rank = made_c;
            c->world = world;
            c->local = g;
            out[made_c] = c;
        }
    }
    if (e != hipSuccess || !barrier_ok || made_c < world) {
        for (int r = 0; r < made_c; ++r) {
            delete out[r];
            out[r] = nullptr;
        }
        if (barrier_ok) pthread_barrier_destroy(&g->barrier);
        for (int k = 0; k < made_ev; ++k) (void)hipEventDestroy(g->ev[k]);
        delete[] g->ev;
        if (g->staging) (void)hipFree(g->staging);
        delete g;
        if (e != hipSuccess) return zf_fail(ZF_ERR_HIP, "zf_comm_create_local_group: %s", hipGetErrorString(e));
        return zf_fail(ZF_ERR_ARG, "zf_comm_create_local_group: out of host memory%s");
    }
    return ZF_OK;
}

extern "C" int zf_comm_destroy(zf_comm* c) {
    if (!c) return ZF_OK;
    if (c->comm) (void)g_rccl.CommDestroy(c->comm);
    if (c->local) {
        zf_local_group* g = c->local;
        pthread_mutex_lock(&g->mu);
        const int left = --g->refs;
        pthread_mutex_unlock(&g->mu);
        if (left == 0) {
            (void)hipDeviceSynchronize();
            for (int k = 0; k < 2 * g->world; ++k) (void)hipEventDestroy(g->ev[k]);
            delete[] g->ev;
            (void)hipFree(g->staging);
            pthread_barrier_destroy(&g->barrier);
            delete g;
        }
    }
    delete c;
    return ZF_OK;
}

extern "C" int zf_comm_info(zf_comm* c, int32_t* rank, int32_t* world) {
    ZF_REQUIRE(c && rank && world, "zf_comm_info: null argument");
    *rank = c->rank;
    *world = c->world;
    return ZF_OK;
}

// What the communicator says about itself: the ranks RCCL reports (ncclCommCount / ncclCommUserRank /
// ncclCommCuDevice - not what the caller passed in), the library the symbols came from, its version, and how many
// all-gathers have gone through it.  A benchmark line built from this shows what RCCL saw.
extern "C" int zf_comm_describe(zf_comm* c, zf_comm_desc* out, int64_t out_bytes) {
    ZF_REQUIRE(out && out_bytes >= (int64_t)sizeof(zf_comm_desc), "zf_comm_describe: out_bytes is smaller than sizeof(zf_comm_desc)");
    ZF_REQUIRE(c, "zf_comm_describe: null communicator");
    memset(out, 0, sizeof(*out));
    out->rank = c->rank;
    out->world = c->world;
    out->kind = c->local ? 1 : 0;
    out->nccl_count = out->nccl_user_rank = out->nccl_device = -1;
    out->all_gathers = c->gathers;
    if (c->comm) {
        int v = 0;
        if (g_rccl.CommCount && g_rccl.CommCount(c->comm, &v) == 0) out->nccl_count = v;
        if (g_rccl.CommUserRank && g_rccl.CommUserRank(c->comm, &v) == 0) out->nccl_user_rank = v;
        if (g_rccl.CommCuDevice && g_rccl.CommCuDevice(c->comm, &v) == 0) out->nccl_device = v;
        if (g_rccl.GetVersion && g_rccl.GetVersion(&v) == 0) out->rccl_version = v;
        snprintf(out->library, sizeof(out->library), "%s", g_rccl.path);
    } else {
        snprintf(out->library, sizeof(out->library), "in-process thread-rank group (no RCCL)");
    }
    return ZF_OK;
}

// recv (world x count doubles, rank-major) <- send (count doubles) of every rank, on `stream`
extern "C" int zf_comm_all_gather(zf_comm* c, const double* send_dev, double* recv_dev, int64_t count, void* stream) {
    ZF_REQUIRE(c && send_dev && recv_dev && count >= 0, "zf_comm_all_gather: bad argument");
    if (c->local) {
        // Every rank thread reaches BOTH barriers whatever happens in between: a failure (a bad count, a HIP error)
        // is remembered, the barriers are met, and only then reported - a rank that returned early would leave the
        // others of the group waiting forever.
        zf_local_group* g = c->local;
        hipError_t e = hipSuccess;
        const bool fits = count <= g->cap;
        const int par = (int)(c->calls++ & 1u);
        double* stage = g->staging + (int64_t)par * g->world * g->cap;
        hipStream_t st = (hipStream_t)stream;
        c->gathers += 1;
        if (fits) {
            e = hipMemcpyAsync(stage + (int64_t)c->rank * count, send_dev, sizeof(double) * count, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(g->ev[par * g->world + c->rank], st);
        }
        // a rank that could not contribute says so BEFORE the first barrier; every rank reads the flag after it: nobody
        // copies out a staging area that holds an older value (and a never re-recorded event) for the failing rank's
        // slice and goes on with stale scalars while only the failing rank reports an error
        if (!fits || e != hipSuccess) __atomic_store_n(&g->failed[par], 1, __ATOMIC_RELEASE);
        pthread_barrier_wait(&g->barrier);   // every rank's copy-in is enqueued and its event recorded
        const bool group_failed = __atomic_load_n(&g->failed[par], __ATOMIC_ACQUIRE) != 0;
        if (fits && e == hipSuccess && !group_failed) {
            for (int r = 0; r < g->world && e == hipSuccess; ++r) e = hipStreamWaitEvent(st, g->ev[par * g->world + r], 0);
            if (e == hipSuccess)
                e = hipMemcpyAsync(recv_dev, stage, sizeof(double) * count * g->world, hipMemcpyDeviceToDevice, st);
        }
        pthread_barrier_wait(&g->barrier);   // nobody re-records an event of this parity before all waits are enqueued
        // (re-armed for the call after next, which every rank starts only after this barrier; the flag of the OTHER
        //  parity is the one the next call uses)
        if (group_failed && c->rank == 0) __atomic_store_n(&g->failed[par], 0, __ATOMIC_RELEASE);
        if (!fits) return zf_fail(ZF_ERR_ARG, "zf_comm_all_gather: count exceeds the local group's staging capacity%s");
        if (e != hipSuccess) return zf_fail(ZF_ERR_HIP, "zf_comm_all_gather (local group): %s", hipGetErrorString(e));
        if (group_failed) return zf_fail(ZF_ERR_STATE, "zf_comm_all_gather (local group): another rank of the group failed in this exchange%s");
        return ZF_OK;
    }
    c->gathers += 1;
    return rccl_check(g_rccl.AllGather(send_dev, recv_dev, (size_t)count, /*ncclDouble*/ 8, c->comm, (hipStream_t)stream),
                      "ncclAllGather");
}
