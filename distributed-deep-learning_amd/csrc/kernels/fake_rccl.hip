// A fake RCCL communicator for ONE process on ONE card: the table behind the override seam of
// rccl_api.h.  It lets the real SyncRunner run as rank r of a world of W > 1 with no peer process
// and no communicator: what the peers would have contributed comes from the test's one-process
// PS simulation (tests/onecard.py simulate_sync), handed over per step as
//
//   peer_grads  [W, total]  every rank's gradient buffer of this step (row `rank` is ignored:
//                           the rank under test contributes its LIVE buffer), and
//   params_next [total]     the parameters every replica must hold after this step.
//
// Every operation is enqueued on the stream the caller gave, as a kernel or an asynchronous
// device copy, and waits for nothing: the runner's own stream order decides what the fake reads
// and when, so that order is what a test of the runner tests, and the fake cannot hang.
//
// THE SUMS ARE IN RANK ORDER, as a left fold from +0 over q = 0 .. W-1.  Real RCCL promises no
// order.  That is deliberate: this pins the RUNNER's arithmetic (which chunk, which root, which
// state offset, which stream), not RCCL's, and it is the order of simulate_sync and of the xGMI
// owner kernels.  What real RCCL does at W > 1 is not measured by anything built on this file.
//
//   ReduceScatter(send, recv, c)  off = send - grads; recv[i] = fold_q (q == rank ?
//                                 send[rank c + i] : peer_grads[q][off + rank c + i])
//   AllGather(send, recv, c)      wants send == recv + rank c (NCCL's in-place form; anything else
//                                 is a violation); copies params_next[off + q c ..] to recv + q c
//                                 for q != rank and leaves the own chunk alone
//   AllReduce(send, recv, n)      in place only; the rank-order sum
//   Reduce(send, recv, n, root)   on the root the rank-order sum into recv; elsewhere nothing
//   Broadcast(send, recv, n, root) on the root nothing; elsewhere recv := params_next[off ..]
//   GroupStart / GroupEnd         a depth counter (nested or unbalanced: a violation)
//   Send / Recv                   a violation (the sync runner has no business calling them)
//
// Peers kPattern serves SyncRunner::selftest, whose scratch buffers are not registered: rank q
// is taken to hold (q + 1) * (i % 13 + 1) at element i, the pattern that self-test documents, and
// an out-of-place AllGather is served as NCCL defines it (the self-test gathers from its shard).
//
// Two lists for the test: every call (op, buffer, offset, count, root, stream, group depth), and
// every violation (a foreign handle, a type other than float32, an op other than sum, a pointer
// or extent outside the registered buffers, a root outside [0, W), the cases above).  A call
// with a violation is logged and NOT executed: nothing is read or written out of bounds.
//
// The fault knob makes the fake wrong on purpose, in data only (no fault, no hang):
//   kRsNextChunk    ReduceScatter reduces chunk (rank + 1) % W
//   kAgSkip         AllGather copies no peer chunk
//   kReduceDropPeer Reduce leaves out the last peer
//   kBcastSkip      Broadcast does nothing on a non-root

#include "fake_rccl.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "rccl_api.h"

namespace ddl {
namespace fake_rccl {
namespace {

struct State {
  std::mutex mu;
  Config cfg;
  const float* peer_grads = nullptr;
  const float* params_next = nullptr;
  int peers = kTable, fault = kNone, depth = 0;
  std::vector<Call> calls;
  std::vector<std::string> bad;
};
State& S() {
  static State s;
  return s;
}
int g_handle;  // its address is the dummy communicator
ncclComm_t handle() { return reinterpret_cast<ncclComm_t>(&g_handle); }

// out[i] = 0 + x_0[i] + x_1[i] + ... in rank order; x_q = own for q == rank (own null: the
// pattern for every rank), else peers[q * stride + i] (peers null: the pattern); `skip` left out
__global__ void __launch_bounds__(256) fold_kernel(float* out, const float* own,
                                                   const float* peers, int64_t stride, int world,
                                                   int rank, int skip, int64_t idx0, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int q = 0; q < world; ++q) {
      if (q == skip) continue;
      float x;
      if (q == rank && own) x = own[i];
      else if (peers) x = peers[q * stride + i];
      else x = (float)((q + 1) * (int)((idx0 + i) % 13 + 1));
      acc = acc + x;
    }
    out[i] = acc;
  }
}

void fold(float* out, const float* own, const float* peers, int skip, int64_t idx0, int64_t n,
          hipStream_t st) {
  if (n <= 0) return;
  State& s = S();
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(fold_kernel, dim3(grid), dim3(256), 0, st, out, own, peers, s.cfg.params.n,
                     s.cfg.world, s.cfg.rank, skip, idx0, n);
}

bool copy(float* dst, const float* src, int64_t n, hipStream_t st) {
  if (n <= 0 || dst == src) return true;
  return hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
}

struct Where {
  std::string name = "other";
  int64_t off = -1, len = 0;
};
Where locate(const void* p) {
  State& s = S();
  const float* f = static_cast<const float*>(p);
  auto in = [&](const Buffer& b) { return b.base && f >= b.base && f < b.base + b.n; };
  if (in(s.cfg.params)) return {"params", f - s.cfg.params.base, s.cfg.params.n};
  if (in(s.cfg.grads)) return {"grads", f - s.cfg.grads.base, s.cfg.grads.n};
  for (size_t k = 0; k < s.cfg.shards.size(); ++k)
    if (in(s.cfg.shards[k]))
      return {"shard" + std::to_string(k), f - s.cfg.shards[k].base, s.cfg.shards[k].n};
  return {};
}

// one call: logged, its common arguments checked.  ok() false: do not execute.
struct Op {
  State& s = S();
  Call c;
  Where snd, rcv;
  bool good = true;
  Op(const char* op, const void* send, void* recv, size_t count, int root, ncclComm_t comm,
     hipStream_t st) {
    snd = locate(send);
    rcv = locate(recv);
    c.op = op;
    c.buf = snd.name, c.off = snd.off;
    c.rbuf = rcv.name, c.roff = rcv.off;
    c.count = (int64_t)count, c.root = root;
    c.stream = reinterpret_cast<uint64_t>(st);
    c.depth = s.depth;
    s.calls.push_back(c);
    if (comm != handle()) fail("a communicator the fake did not make");
  }
  void fail(const std::string& why) {
    good = false;
    s.bad.push_back(c.op + ": " + why);
  }
  void type(ncclDataType_t t) {
    if (t != ncclFloat32) fail("datatype other than float32");
  }
  void sum(ncclRedOp_t o) {
    if (o != ncclSum) fail("reduction other than sum");
  }
  void root() {
    if (c.root < 0 || c.root >= s.cfg.world) fail("root outside [0, W)");
  }
  // kTable: the side lies in buffer `name` with `extent` elements from its offset
  void inside(const Where& w, const char* name, bool shard, int64_t extent, const char* side) {
    if (s.peers != kTable) return;
    const bool right = shard ? w.name.rfind("shard", 0) == 0 : w.name == name;
    if (!right || w.off + extent > w.len)
      fail(std::string(side) + " pointer or extent outside " + name);
  }
  void table(bool need_grads, bool need_params) {
    if (s.peers != kTable) return;
    if ((need_grads && !s.peer_grads) || (need_params && !s.params_next))
      fail("no step data (set_step)");
  }
  // every reduction's send range as the rank under test held it
  void keep_seen(const float* send, int64_t n, hipStream_t st) {
    if (good && s.peers == kTable && s.cfg.seen) (void)copy(s.cfg.seen + snd.off, send, n, st);
  }
};

#define LOCKED std::lock_guard<std::mutex> lock_(S().mu)

ncclResult_t GetUniqueId(ncclUniqueId* id) {
  memset(id, 0, sizeof(*id));
  return ncclSuccess;
}
ncclResult_t CommInitRank(ncclComm_t* comm, int world, ncclUniqueId, int rank) {
  LOCKED;
  State& s = S();
  if (world != s.cfg.world || rank != s.cfg.rank)
    s.bad.push_back("CommInitRank: world / rank differ from the configured ones");
  *comm = handle();
  return ncclSuccess;
}
ncclResult_t CommDestroy(ncclComm_t c) {
  LOCKED;
  if (c != handle()) S().bad.push_back("CommDestroy: a communicator the fake did not make");
  return ncclSuccess;
}
ncclResult_t CommAbort(ncclComm_t c) { return CommDestroy(c); }
const char* GetErrorString(ncclResult_t) { return "fake RCCL error"; }
ncclResult_t CommGetAsyncError(ncclComm_t c, ncclResult_t* out) {
  LOCKED;
  if (c != handle()) S().bad.push_back("CommGetAsyncError: a communicator the fake did not make");
  *out = ncclSuccess;
  return ncclSuccess;
}

ncclResult_t ReduceScatter(const void* send, void* recv, size_t count, ncclDataType_t t,
                           ncclRedOp_t o, ncclComm_t comm, hipStream_t st) {
  LOCKED;
  Op op("ReduceScatter", send, recv, count, -1, comm, st);
  State& s = op.s;
  const int64_t c = (int64_t)count, W = s.cfg.world;
  op.type(t), op.sum(o);
  op.inside(op.snd, "grads", false, W * c, "send");
  op.inside(op.rcv, "a shard buffer", true, c, "recv");
  op.table(true, false);
  if (!op.good) return ncclSuccess;
  const float* sf = static_cast<const float*>(send);
  op.keep_seen(sf, W * c, st);
  const int64_t chunk = s.fault == kRsNextChunk ? (s.cfg.rank + 1) % W : s.cfg.rank;
  const float* peers = s.peers == kTable ? s.peer_grads + op.snd.off + chunk * c : nullptr;
  fold(static_cast<float*>(recv), sf + chunk * c, peers, -1, chunk * c, c, st);
  return ncclSuccess;
}

ncclResult_t AllGather(const void* send, void* recv, size_t count, ncclDataType_t t,
                       ncclComm_t comm, hipStream_t st) {
  LOCKED;
  Op op("AllGather", send, recv, count, -1, comm, st);
  State& s = op.s;
  const int64_t c = (int64_t)count, W = s.cfg.world, r = s.cfg.rank;
  float* rf = static_cast<float*>(recv);
  const float* sf = static_cast<const float*>(send);
  op.type(t);
  op.inside(op.rcv, "params", false, W * c, "recv");
  op.table(false, true);
  const bool in_place = sf == rf + r * c;
  if (s.peers == kTable && !in_place) op.fail("not in place (send != recv + rank * count)");
  if (!op.good) return ncclSuccess;
  bool ok = in_place || copy(rf + r * c, sf, c, st);
  for (int64_t q = 0; q < W && s.fault != kAgSkip; ++q) {
    if (q == r) continue;
    if (s.peers == kTable) ok &= copy(rf + q * c, s.params_next + op.rcv.off + q * c, c, st);
    else fold(rf + q * c, nullptr, nullptr, -1, q * c, c, st);
  }
  return ok ? ncclSuccess : ncclUnhandledCudaError;
}

ncclResult_t AllReduce(const void* send, void* recv, size_t count, ncclDataType_t t,
                       ncclRedOp_t o, ncclComm_t comm, hipStream_t st) {
  LOCKED;
  Op op("AllReduce", send, recv, count, -1, comm, st);
  State& s = op.s;
  const int64_t n = (int64_t)count;
  op.type(t), op.sum(o);
  op.inside(op.snd, "grads", false, n, "send");
  op.table(true, false);
  if (send != recv) op.fail("not in place");
  if (!op.good) return ncclSuccess;
  const float* sf = static_cast<const float*>(send);
  op.keep_seen(sf, n, st);
  fold(static_cast<float*>(recv), sf, s.peers == kTable ? s.peer_grads + op.snd.off : nullptr, -1,
       0, n, st);
  return ncclSuccess;
}

ncclResult_t Reduce(const void* send, void* recv, size_t count, ncclDataType_t t, ncclRedOp_t o,
                    int root, ncclComm_t comm, hipStream_t st) {
  LOCKED;
  Op op("Reduce", send, recv, count, root, comm, st);
  State& s = op.s;
  const int64_t n = (int64_t)count;
  op.type(t), op.sum(o), op.root();
  op.inside(op.snd, "grads", false, n, "send");
  if (root == s.cfg.rank) op.inside(op.rcv, "grads", false, n, "recv");
  op.table(true, false);
  if (!op.good) return ncclSuccess;
  const float* sf = static_cast<const float*>(send);
  op.keep_seen(sf, n, st);
  if (root != s.cfg.rank) return ncclSuccess;
  int skip = -1;
  if (s.fault == kReduceDropPeer)
    skip = s.cfg.rank == s.cfg.world - 1 ? s.cfg.world - 2 : s.cfg.world - 1;
  fold(static_cast<float*>(recv), sf, s.peers == kTable ? s.peer_grads + op.snd.off : nullptr,
       skip, 0, n, st);
  return ncclSuccess;
}

ncclResult_t Broadcast(const void* send, void* recv, size_t count, ncclDataType_t t, int root,
                       ncclComm_t comm, hipStream_t st) {
  LOCKED;
  Op op("Broadcast", send, recv, count, root, comm, st);
  State& s = op.s;
  const int64_t n = (int64_t)count;
  op.type(t), op.root();
  op.inside(op.rcv, "params", false, n, "recv");
  op.table(false, true);
  if (!op.good || root == s.cfg.rank || s.fault == kBcastSkip) return ncclSuccess;
  float* rf = static_cast<float*>(recv);
  if (s.peers == kTable)
    return copy(rf, s.params_next + op.rcv.off, n, st) ? ncclSuccess : ncclUnhandledCudaError;
  fold(rf, nullptr, nullptr, -1, 0, n, st);
  return ncclSuccess;
}

ncclResult_t Send(const void* send, size_t count, ncclDataType_t, int peer, ncclComm_t comm,
                  hipStream_t st) {
  LOCKED;
  Op op("Send", send, nullptr, count, peer, comm, st);
  op.fail("point-to-point call from the sync runner");
  return ncclSuccess;
}
ncclResult_t Recv(void* recv, size_t count, ncclDataType_t, int peer, ncclComm_t comm,
                  hipStream_t st) {
  LOCKED;
  Op op("Recv", nullptr, recv, count, peer, comm, st);
  op.fail("point-to-point call from the sync runner");
  return ncclSuccess;
}

ncclResult_t Group(const char* name, int step) {
  LOCKED;
  State& s = S();
  Call c;
  c.op = name;
  c.depth = s.depth;
  s.calls.push_back(c);
  s.depth += step;
  if (s.depth > 1) s.bad.push_back("GroupStart: nested group");
  if (s.depth < 0) {
    s.bad.push_back("GroupEnd: no group open");
    s.depth = 0;
  }
  return ncclSuccess;
}
ncclResult_t GroupStart() { return Group("GroupStart", 1); }
ncclResult_t GroupEnd() { return Group("GroupEnd", -1); }

const RcclApi& the_table() {
  static const RcclApi api = [] {
    RcclApi a;
    a.GetUniqueId = GetUniqueId;
    a.CommInitRank = CommInitRank;
    a.CommDestroy = CommDestroy;
    a.GetErrorString = GetErrorString;
    a.ReduceScatter = ReduceScatter;
    a.AllGather = AllGather;
    a.AllReduce = AllReduce;
    a.Reduce = Reduce;
    a.Broadcast = Broadcast;
    a.Send = Send;
    a.Recv = Recv;
    a.GroupStart = GroupStart;
    a.GroupEnd = GroupEnd;
    a.CommGetAsyncError = CommGetAsyncError;
    a.CommAbort = CommAbort;
    return a;
  }();
  return api;
}

}  // namespace

void install(const Config& c) {
  if (c.world < 1 || c.rank < 0 || c.rank >= c.world)
    throw std::invalid_argument("fake RCCL: rank outside [0, world)");
  if (!c.params.base || !c.grads.base || c.params.n != c.grads.n || c.params.n <= 0)
    throw std::invalid_argument("fake RCCL: params and grads of one length");
  set_rccl_override(&the_table());  // (throws while a communicator lives: nothing changed then)
  LOCKED;
  State& s = S();
  s.cfg = c;
  s.peer_grads = s.params_next = nullptr;
  s.peers = kTable, s.fault = kNone, s.depth = 0;
  s.calls.clear();
  s.bad.clear();
}

void remove() {
  set_rccl_override(nullptr);
  LOCKED;
  State& s = S();
  s.cfg = Config();
  s.peer_grads = s.params_next = nullptr;
}

void set_step(const float* peer_grads, const float* params_next) {
  LOCKED;
  S().peer_grads = peer_grads;
  S().params_next = params_next;
}
void set_peers(int peers) {
  if (peers != kTable && peers != kPattern) throw std::invalid_argument("fake RCCL: peers");
  LOCKED;
  S().peers = peers;
}
void set_fault(int fault) {
  if (fault < kNone || fault > kBcastSkip) throw std::invalid_argument("fake RCCL: fault");
  LOCKED;
  S().fault = fault;
}
void clear() {
  LOCKED;
  S().calls.clear();
  S().bad.clear();
}
std::vector<Call> calls() {
  LOCKED;
  return S().calls;
}
std::vector<std::string> violations() {
  LOCKED;
  return S().bad;
}
int group_depth() {
  LOCKED;
  return S().depth;
}
bool overridden() { return rccl_overridden(); }

}  // namespace fake_rccl
}  // namespace ddl
