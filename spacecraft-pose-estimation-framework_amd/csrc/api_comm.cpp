// RCCL: communicators with bounded waits and the collective weight broadcast (include/spef.h).
#include <rccl/rccl.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>
#include <thread>

#include "spef_ctx.hpp"

extern "C" {

#define NCCL_TRY(expr)                                                                                      \
  do {                                                                                                      \
    ncclResult_t r_ = (expr);                                                                               \
    if (r_ != ncclSuccess) return fail(SPEF_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(r_));  \
  } while (0)

// Communicators made by spef_comm_init: nonblocking (ncclConfig_t.blocking = 0) with a per-communicator timeout, so
// every wait below is bounded and a dead peer ends in ncclCommAbort instead of a hang. A communicator
// the host made itself is unknown here and gets kDefaultCommTimeoutMs.
namespace {
const int kDefaultCommTimeoutMs = 120000;
struct CommInfo {
  int timeout_ms;
  bool aborted;
};
std::mutex g_comm_mu;
std::map<void*, CommInfo> g_comms;

int comm_timeout(void* comm) {
  std::lock_guard<std::mutex> g(g_comm_mu);
  auto it = g_comms.find(comm);
  return it == g_comms.end() ? kDefaultCommTimeoutMs : it->second.timeout_ms;
}

using Clock = std::chrono::steady_clock;

// Abort the communicator (unblocks every kernel of it on this rank; the handle is dead afterwards) and fail.
int comm_abort_fail(ncclComm_t comm, const std::string& msg) {
  ncclCommAbort(comm);
  {
    std::lock_guard<std::mutex> g(g_comm_mu);
    auto it = g_comms.find((void*)comm);
    if (it != g_comms.end()) it->second.aborted = true;
    else g_comms[(void*)comm] = {kDefaultCommTimeoutMs, true};
  }
  return fail(SPEF_ERR_COMM, msg + " -- communicator aborted (ncclCommAbort)");
}

// Wait until a nonblocking RCCL call has left ncclInProgress; abort on error or at the deadline.
int comm_settle(ncclComm_t comm, ncclResult_t r, Clock::time_point deadline, const char* what) {
  while (r == ncclInProgress) {
    if (Clock::now() > deadline) return comm_abort_fail(comm, std::string(what) + ": timed out");
    std::this_thread::sleep_for(std::chrono::microseconds(50));
    if (ncclCommGetAsyncError(comm, &r) != ncclSuccess) r = ncclSystemError;
  }
  if (r != ncclSuccess) return comm_abort_fail(comm, std::string(what) + ": " + ncclGetErrorString(r));
  return SPEF_OK;
}

// Wait for the stream's collectives to finish, polling the communicator's async error; abort at the deadline.
int comm_wait_stream(ncclComm_t comm, hipStream_t s, Clock::time_point deadline, const char* what, int inject) {
  for (;;) {
    const hipError_t e = inject ? hipErrorNotReady : hipStreamQuery(s);
    if (e == hipSuccess) return SPEF_OK;
    if (e != hipErrorNotReady) return comm_abort_fail(comm, std::string(what) + ": " + hipGetErrorString(e));
    ncclResult_t ae = ncclSuccess;
    if (ncclCommGetAsyncError(comm, &ae) != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress))
      return comm_abort_fail(comm, std::string(what) + ": " + ncclGetErrorString(ae));
    if (Clock::now() > deadline) return comm_abort_fail(comm, std::string(what) + ": timed out");
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}
}  // namespace

int spef_comm_unique_id(void* id_out, size_t cap) {
  if (!id_out || cap < sizeof(ncclUniqueId)) return fail(SPEF_ERR_ARG, "id buffer smaller than SPEF_COMM_ID_BYTES");
  static_assert(sizeof(ncclUniqueId) == SPEF_COMM_ID_BYTES, "SPEF_COMM_ID_BYTES != sizeof(ncclUniqueId)");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(id_out, &id, sizeof(id));
  return SPEF_OK;
}

int spef_comm_init(int device, int nranks, int rank, const void* id, int timeout_ms, void** comm_out) {
  if (!id || !comm_out || nranks < 1 || rank < 0 || rank >= nranks) return fail(SPEF_ERR_ARG, "bad communicator arguments");
  if (timeout_ms <= 0) timeout_ms = kDefaultCommTimeoutMs;
  Dev d(device);
  HIP_TRY(hipSetDevice(device));
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  ncclComm_t comm = nullptr;
  ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
  cfg.blocking = 0;
  const ncclResult_t r = ncclCommInitRankConfig(&comm, nranks, uid, rank, &cfg);
  if (r != ncclSuccess && r != ncclInProgress) return fail(SPEF_ERR_COMM, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r));
  {
    std::lock_guard<std::mutex> g(g_comm_mu);
    g_comms[(void*)comm] = {timeout_ms, false};
  }
  const int rc = comm_settle(comm, r, Clock::now() + std::chrono::milliseconds(timeout_ms), "communicator init");
  if (rc) {   // aborted: the handle is gone
    std::lock_guard<std::mutex> g(g_comm_mu);
    g_comms.erase((void*)comm);
    return rc;
  }
  *comm_out = comm;
  return SPEF_OK;
}

int spef_comm_abort(void* comm) {
  if (!comm) return SPEF_OK;
  {
    std::lock_guard<std::mutex> g(g_comm_mu);
    auto it = g_comms.find(comm);
    if (it != g_comms.end() && it->second.aborted) return SPEF_OK;
  }
  comm_abort_fail((ncclComm_t)comm, "spef_comm_abort");
  return SPEF_OK;
}

int spef_comm_destroy(void* comm) {
  if (!comm) return SPEF_OK;
  bool aborted = false;
  {
    std::lock_guard<std::mutex> g(g_comm_mu);
    auto it = g_comms.find(comm);
    if (it != g_comms.end()) {
      aborted = it->second.aborted;
      g_comms.erase(it);
    }
  }
  if (aborted) return SPEF_OK;   // ncclCommAbort already released it
  ncclComm_t cm = (ncclComm_t)comm;
  const Clock::time_point dl = Clock::now() + std::chrono::milliseconds(kDefaultCommTimeoutMs);
  ncclResult_t r = ncclCommFinalize(cm);   // nonblocking communicators finalize asynchronously
  if (r == ncclInProgress) {
    while (r == ncclInProgress && Clock::now() < dl) {
      std::this_thread::sleep_for(std::chrono::microseconds(50));
      if (ncclCommGetAsyncError(cm, &r) != ncclSuccess) r = ncclSystemError;
    }
  }
  if (r != ncclSuccess) {
    ncclCommAbort(cm);
    return fail(SPEF_ERR_COMM, std::string("ncclCommFinalize: ") + ncclGetErrorString(r) + " -- aborted");
  }
  NCCL_TRY(ncclCommDestroy(cm));
  return SPEF_OK;
}

// Collective weight broadcast with agreement: no rank enters a data collective unless every rank reported a good
// local state, and every rank returns the same verdict. Steps: header broadcast -> local checks + allocation ->
// all-reduce(MAX) of the status words -> op table + data broadcasts -> receivers stage (parse, copy, validate) ->
// second all-reduce(MAX) -> receivers commit. Any RCCL error or a wait past the communicator's timeout aborts the
// communicator (ncclCommAbort) and returns SPEF_ERR_COMM; a failing rank is named in spef_last_error on every rank.
// Status word: 0 = ok, else (error code << 16) | (failing rank + 1); MAX picks one failing rank deterministically.
int spef_bcast_weights(spef_ctx* c, void* comm_, int root) {
  if (!c || !comm_) return fail(SPEF_ERR_ARG, "null argument");
  ncclComm_t comm = (ncclComm_t)comm_;
  {
    std::lock_guard<std::mutex> g(g_comm_mu);
    auto it = g_comms.find(comm_);
    if (it != g_comms.end() && it->second.aborted) return fail(SPEF_ERR_COMM, "communicator was aborted");
  }
  int rank = 0, n = 0;
  NCCL_TRY(ncclCommUserRank(comm, &rank));
  NCCL_TRY(ncclCommCount(comm, &n));
  if (root < 0 || root >= n) return fail(SPEF_ERR_ARG, "root out of range");
  Dev d(c->device);
  const Clock::time_point deadline = Clock::now() + std::chrono::milliseconds(comm_timeout(comm_));
  const int inject = c->test_fail_bcast;   // spef_tuning.hpp SPEF_OPT_TEST_FAIL_BCAST
  struct Tmp {   // scratch freed on every exit path
    hipStream_t s = nullptr;
    uint8_t* hdr = nullptr;
    uint8_t* img = nullptr;
    int32_t* st = nullptr;
    ~Tmp() {   // (after an abort the communicator's kernels have been told to exit)
      if (s) hipStreamDestroy(s);
      if (hdr) hipFree(hdr);
      if (img) hipFree(img);
      if (st) hipFree(st);
    }
  } t;
  HIP_TRY(hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&t.hdr, sizeof(BlobHeader)));
  HIP_TRY(hipMalloc(&t.st, sizeof(int32_t)));
  int rc;
#define COMM_CALL(expr, what)                                                        \
  do {                                                                               \
    if ((rc = comm_settle(comm, (expr), deadline, what)) != SPEF_OK) return rc;      \
  } while (0)
#define COMM_WAIT(what, inj)                                                         \
  do {                                                                               \
    if ((rc = comm_wait_stream(comm, t.s, deadline, what, inj)) != SPEF_OK) return rc; \
  } while (0)
  // agree on a local status word; returns the MAX over ranks (or an error: communicator aborted)
  std::string local_msg;
  auto agree = [&](int local_code, int32_t* agreed, int inj) -> int {
    const int32_t w = local_code ? (int32_t)((local_code << 16) | (rank + 1)) : 0;
    HIP_TRY(hipMemcpyAsync(t.st, &w, sizeof(w), hipMemcpyHostToDevice, t.s));
    COMM_CALL(ncclAllReduce(t.st, t.st, 1, ncclInt32, ncclMax, comm, t.s), "status all-reduce");
    COMM_WAIT("status all-reduce", inj);
    HIP_TRY(hipMemcpy(agreed, t.st, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SPEF_OK;
  };
  auto verdict = [&](int32_t agreed) -> int {
    const int code = agreed >> 16, bad = (agreed & 0xffff) - 1;
    if (bad == rank) return fail(code, local_msg + " (rank " + std::to_string(rank) + ", weight broadcast)");
    return fail(code, "weight broadcast failed on rank " + std::to_string(bad) + " (error " + std::to_string(code) +
                          "); every rank returns it and keeps its previous model");
  };

  // 1. header (a root without weights sends an all-zero header; the receivers' checks then fail together)
  BlobHeader h{};
  if (rank == root && c->loaded) h = c->hdr;
  HIP_TRY(hipMemcpy(t.hdr, &h, sizeof(h), hipMemcpyHostToDevice));
  COMM_CALL(ncclBroadcast(t.hdr, t.hdr, sizeof(h), ncclUint8, root, comm, t.s), "header broadcast");
  COMM_WAIT("header broadcast", inject == 3);
  HIP_TRY(hipMemcpy(&h, t.hdr, sizeof(h), hipMemcpyDeviceToHost));

  // 2. local checks and allocation, then agreement before any bulk collective
  int local = SPEF_OK;
  const size_t ops_bytes = (size_t)h.n_ops * sizeof(OpDesc);
  if (memcmp(h.magic, kBlobMagic, 8) != 0) {
    local = fail(SPEF_ERR_STATE, "broadcast root has no weights loaded");
  } else if (h.data_off > (1ull << 30) || h.data_bytes > (1ull << 36) || h.ops_off > h.data_off ||
             ops_bytes > h.data_off - h.ops_off) {
    local = fail(SPEF_ERR_BLOB, "broadcast header out of range");
  } else if (inject == 1) {
    local = fail(SPEF_ERR_HIP, "injected failure before the data broadcast (SPEF_OPT_TEST_FAIL_BCAST=1)");
  } else if (rank != root) {
    const size_t total = (size_t)h.data_off + (size_t)h.data_bytes;
    const hipError_t e = hipMalloc(&t.img, std::max<size_t>(total, 256));
    if (e != hipSuccess) {
      t.img = nullptr;
      local = fail(SPEF_ERR_HIP, std::string("hipMalloc of the broadcast image: ") + hipGetErrorString(e));
    }
  }
  if (local) local_msg = spef_last_error();
  int32_t agreed = 0;
  if ((rc = agree(local, &agreed, 0)) != SPEF_OK) return rc;
  if (agreed) return verdict(agreed);

  // 3. op table + data section (receivers: into a full blob image they then stage like spef_load_weights_device)
  if (rank == root) {
    HIP_TRY(hipMalloc(&t.img, std::max<size_t>(ops_bytes, 256)));
    HIP_TRY(hipMemcpy(t.img, c->ops.data(), ops_bytes, hipMemcpyHostToDevice));
    COMM_CALL(ncclGroupStart(), "group start");
    COMM_CALL(ncclBroadcast(t.img, t.img, ops_bytes, ncclUint8, root, comm, t.s), "op-table broadcast");
    COMM_CALL(ncclBroadcast(c->d_data, c->d_data, h.data_bytes, ncclUint8, root, comm, t.s), "data broadcast");
    COMM_CALL(ncclGroupEnd(), "group end");
  } else {
    HIP_TRY(hipMemcpy(t.img, &h, sizeof(h), hipMemcpyHostToDevice));
    COMM_CALL(ncclGroupStart(), "group start");
    COMM_CALL(ncclBroadcast(t.img + h.ops_off, t.img + h.ops_off, ops_bytes, ncclUint8, root, comm, t.s),
              "op-table broadcast");
    COMM_CALL(ncclBroadcast(t.img + h.data_off, t.img + h.data_off, h.data_bytes, ncclUint8, root, comm, t.s),
              "data broadcast");
    COMM_CALL(ncclGroupEnd(), "group end");
  }
  COMM_WAIT("data broadcast", 0);

  // 4. receivers stage (full validation + device copy); all ranks agree before anyone commits
  Staged st;
  local = SPEF_OK;
  if (inject == 2) local = fail(SPEF_ERR_BLOB, "injected failure after the data broadcast (SPEF_OPT_TEST_FAIL_BCAST=2)");
  else if (rank != root) local = stage_blob(c, t.img, (size_t)h.data_off + (size_t)h.data_bytes, true, &st);
  local_msg = local ? std::string(spef_last_error()) : std::string();
  if ((rc = agree(local, &agreed, 0)) != SPEF_OK) return rc;
  if (agreed) return verdict(agreed);
  if (rank != root) commit_staged(c, &st);   // the root keeps its loaded model
  return SPEF_OK;
#undef COMM_CALL
#undef COMM_WAIT
}

}  // extern "C"
