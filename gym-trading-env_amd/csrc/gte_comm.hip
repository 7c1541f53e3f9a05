// gte_comm.hip — the ONE exchange step of the sharded path: the RCCL all-gather of the per-step
// returns (reward f32 | terminated u8 | truncated u8 = 6 bytes per env, which the step kernel
// writes in exactly that packed layout) and, on request, of the observations, called from inside
// the library so that a C caller of libgte has a multi-GPU path and a per-step gather costs no
// framework overhead (SURVEY §8b `gte_allgather`, §8e).
//
// RCCL is bound at run time (dlopen of the librccl already in the process — PyTorch's when the
// host layer is Python — else the system one): libgte.so itself has no link-time dependency on
// it and loads on hosts without RCCL.  One communicator per env, created from an id the caller
// distributes (rank 0: gte_comm_unique_id; every rank: gte_comm_init).
//
// Modes of a gather (gte.h): 0 = on the env's stream, i.e. stream-ordered between two steps
// (the synchronous per-step form: step t -> gather t -> step t+1, no host synchronisation);
// 1 = on the library's communication stream behind an event recorded on the env's stream, so
// that the steps enqueued afterwards overlap it (the caller rotates return buffers with
// gte_bind_returns / gathers whole blocks of rows, and joins with gte_comm_wait).
//
// On the fully connected 7-link xGMI topology the direct (one-shot) all-gather moves each
// shard over all links at once, where a ring is bound by one link per hop; which
// one RCCL uses is RCCL's choice, steerable from outside with NCCL_ALGO / NCCL_PROTO
//  — the payload here is 6 bytes per env, far below either limit.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include "gte_host.h"  // (with <cstdio>, <cstring>, <string>)

namespace gte {

struct RcclApi {
  void* handle = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string error;
};

static RcclApi& rccl() {
  static RcclApi api;
  return api;
}

// -> nullptr on success, else why RCCL is not usable
const char* rccl_load() {
  RcclApi& a = rccl();
  if (a.AllGather) return nullptr;
  const char* names[] = {"librccl.so.1", "librccl.so"};
  // a copy already loaded into the process first (two RCCLs in one process would each keep
  // their own view of the devices), then a fresh load
  for (int pass = 0; pass < 2 && !a.handle; ++pass)
    for (const char* n : names) {
      a.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
      if (a.handle) break;
    }
  if (!a.handle) a.handle = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!a.handle) {
    a.error = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?");
    return a.error.c_str();
  }
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(a.handle, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(a.handle, "ncclCommInitRank");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.handle, "ncclCommDestroy");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.handle, "ncclGetErrorString");
  a.AllGather = (decltype(a.AllGather))dlsym(a.handle, "ncclAllGather");
  if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.GetErrorString || !a.AllGather) {
    a.AllGather = nullptr;
    a.error = "librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclAllGather / "
              "ncclCommDestroy / ncclGetErrorString";
    return a.error.c_str();
  }
  return nullptr;
}

const char* rccl_error(int code) { return rccl().GetErrorString((ncclResult_t)code); }

int rccl_unique_id(uint8_t* out128) {
  ncclUniqueId id;
  const ncclResult_t r = rccl().GetUniqueId(&id);
  if (r == ncclSuccess) memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
  return (int)r;
}

int rccl_comm_init(void** comm, const uint8_t* id128, int rank, int world) {
  ncclUniqueId id;
  memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t c = nullptr;
  const ncclResult_t r = rccl().CommInitRank(&c, world, id, rank);
  *comm = (void*)c;
  return (int)r;
}

int rccl_allgather_bytes(void* comm, const void* src, void* dst, size_t bytes, hipStream_t stream) {
  return (int)rccl().AllGather(src, dst, bytes, ncclUint8, (ncclComm_t)comm, stream);
}

int rccl_comm_destroy(void* comm) { return (int)rccl().CommDestroy((ncclComm_t)comm); }

}  // namespace gte

extern "C" {  // the entry points of include/gte.h that use the wrappers above

int gte_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(GTE_ERR_INVALID, "id_out is NULL");
  if (const char* why = gte::rccl_load()) return fail(GTE_ERR_STATE, "RCCL unavailable: %s", why);
  const int r = gte::rccl_unique_id(id_out);
  if (r != 0) return fail(GTE_ERR_HIP, "ncclGetUniqueId: %s", gte::rccl_error(r));
  return GTE_OK;
}

int gte_comm_init(gte_env* E, const uint8_t* id, int32_t rank, int32_t world) {
  if (!E || !id) return fail(GTE_ERR_INVALID, "NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(GTE_ERR_INVALID, "rank %d of %d", rank, world);
  if (E->comm.handle) return fail(GTE_ERR_STATE, "the env already has a communicator");
  if (const char* why = gte::rccl_load()) return fail(GTE_ERR_STATE, "RCCL unavailable: %s", why);
  HIPCHK(hipSetDevice(E->cfg.device));
  const int r = gte::rccl_comm_init(&E->comm.handle, id, rank, world);
  if (r != 0) { E->comm.handle = nullptr; return fail(GTE_ERR_HIP, "ncclCommInitRank: %s", gte::rccl_error(r)); }
  E->comm.rank = rank;
  E->comm.world = world;
  // anything failing from here on must not leave a half-made communicator behind (a retry would
  // be refused with "already has a communicator"): undo everything, keep the error message
  auto finish = [&]() -> int {
    HIPCHK(hipStreamCreateWithFlags(&E->comm.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&E->comm.ready, hipEventDisableTiming));
    for (auto& ev : E->comm.done) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    E->comm.gathered_returns.reset();  // a communicator of another size was here before
    const size_t bytes = (size_t)world * 6 * (size_t)E->p.N;
    TRY(device_alloc(&E->comm.gathered_returns, bytes, "gathered returns (%d ranks x %d envs): %s", world, E->p.N));
    HIPCHK(hipMemset(E->comm.gathered_returns.get(), 0, bytes));
    HIPCHK(hipDeviceSynchronize());
    return GTE_OK;
  };
  const int rc = finish();
  if (rc != GTE_OK) {
    const std::string keep = g_err;
    (void)gte_comm_destroy(E);
    g_err = keep;
  }
  return rc;
}

int gte_allgather(gte_env* E, const void* src_device, void* dst_device, uint64_t bytes_per_rank,
                  int32_t mode) {
  if (!E || !src_device || !dst_device) return fail(GTE_ERR_INVALID, "NULL argument");
  if (!E->comm.handle) return fail(GTE_ERR_STATE, "gte_allgather before gte_comm_init");
  if (mode != 0 && mode != 1) return fail(GTE_ERR_INVALID, "mode must be 0 (env stream) or 1 (overlapped)");
  hipStream_t s = E->stream;
  if (mode == 1) {  // behind everything enqueued so far, beside everything enqueued later
    HIPCHK(hipEventRecord(E->comm.ready, E->stream));
    HIPCHK(hipStreamWaitEvent(E->comm.stream, E->comm.ready, 0));
    s = E->comm.stream;
  }
  const int r = gte::rccl_allgather_bytes(E->comm.handle, src_device, dst_device, (size_t)bytes_per_rank, s);
  if (r != 0) return fail(GTE_ERR_HIP, "ncclAllGather: %s", gte::rccl_error(r));
  if (mode == 1) {
    HIPCHK(hipEventRecord(E->comm.done[E->comm.seq & 3], E->comm.stream));
    E->comm.seq += 1;
  }
  return GTE_OK;
}

int gte_allgather_returns(gte_env* E, void* dst_device, int32_t mode, const void** gathered) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->comm.handle) return fail(GTE_ERR_STATE, "gte_allgather_returns before gte_comm_init");
  const Params& p = E->p;
  const size_t N = (size_t)p.N;
  if ((const uint8_t*)p.terminated != (const uint8_t*)p.reward + 4 * N || p.truncated != p.terminated + N)
    return fail(GTE_ERR_STATE, "the bound return buffers are not one packed [reward f32 | terminated u8 "
                               "| truncated u8] block of 6N bytes");
  void* dst = dst_device ? dst_device : E->comm.gathered_returns.get();
  TRY(gte_allgather(E, p.reward, dst, 6 * N, mode));
  if (gathered) *gathered = dst;
  return GTE_OK;
}

int gte_allgather_obs(gte_env* E, float* dst_device, int32_t mode) {
  if (!E || !dst_device) return fail(GTE_ERR_INVALID, "NULL argument");
  const Params& p = E->p;
  if (!p.obs) return fail(GTE_ERR_STATE, "gte_allgather_obs before gte_reset (no observation exists yet)");
  if (E->sliding)
    return fail(GTE_ERR_STATE, "gte_allgather_obs on a sliding observation buffer: the windows are not contiguous "
                               "(bind a classic buffer with gte_bind_outputs first)");
  return gte_allgather(E, p.obs, dst_device, sizeof(float) * (size_t)p.N * p.W * p.Fobs, mode);
}

int gte_comm_wait(gte_env* E, int32_t back) {
  if (!E || !E->comm.handle) return fail(GTE_ERR_STATE, "no communicator");
  if (back < 0 || back > 3) return fail(GTE_ERR_INVALID, "back must be 0..3");
  const int64_t k = E->comm.seq - 1 - back;  // the overlapped gather to wait for
  if (k < 0) return GTE_OK;                  // not issued yet: nothing to wait for
  HIPCHK(hipStreamWaitEvent(E->stream, E->comm.done[k & 3], 0));
  return GTE_OK;
}

int gte_comm_synchronize(gte_env* E) {
  if (!E || !E->comm.handle) return fail(GTE_ERR_STATE, "no communicator");
  HIPCHK(hipStreamSynchronize(E->comm.stream));
  return GTE_OK;
}

int gte_comm_destroy(gte_env* E) {
  if (!E) return fail(GTE_ERR_INVALID, "env is NULL");
  if (!E->comm.handle) return GTE_OK;
  (void)hipStreamSynchronize(E->stream);
  if (E->comm.stream) (void)hipStreamSynchronize(E->comm.stream);
  const int r = gte::rccl_comm_destroy(E->comm.handle);
  E->comm.handle = nullptr;
  if (E->comm.ready) (void)hipEventDestroy(E->comm.ready);
  for (auto& ev : E->comm.done) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
  if (E->comm.stream) (void)hipStreamDestroy(E->comm.stream);
  E->comm.ready = nullptr;
  E->comm.seq = 0;
  E->comm.stream = nullptr;
  if (r != 0) return fail(GTE_ERR_HIP, "ncclCommDestroy: %s", gte::rccl_error(r));
  return GTE_OK;
}

}  // extern "C"
