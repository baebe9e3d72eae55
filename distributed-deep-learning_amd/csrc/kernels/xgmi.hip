// Parameter-server exchange over xGMI peer memory: one kernel per gradient bucket does the
// whole synchronous PS round trip of SURVEY.md §2.7 for the byte-equal flat plan — push the
// gradient chunks to their owners, sum at the owner, Adam on the owner's shard, push the new
// parameters back to every worker — with remote stores into IPC-mapped peer buffers instead
// of RCCL's reduce-scatter + all-gather (two collective launches, a ring pass each).
//
// Reference behaviour being replaced: every worker Sends each gradient tensor to the owning
// PS, the PS sums the W arrivals with NumPy and runs ApplyAdam, then Sends the parameters back
// (mnist_sync_sharding/worker.py:30-37,88-94; parameter_server.py:76-82,108-126).
//
// Why a kernel of our own (MI355X): the 8 GPUs of a node are a full xGMI mesh (7 links per GPU),
// so the owner of chunk r can receive its W-1 gradient pieces on W-1 different links at once,
// and a store to a peer's HBM is posted (no round trip).  One launch per bucket with a few dozen
// workgroups leaves the CUs to the backward GEMMs it overlaps with; all traffic is writes.
//
// Protocol (per bucket b, step epoch e; workgroup j owns slice j of every rank's chunk):
//   phase 1  for every owner r != me: store grads[b][chunk r][slice j] -> inbox_r[b][me][slice j]
//            (write-through, system scope), drain, then ARRIVE_r[b][me][j] = e
//   phase 2  wait ARRIVE_me[b][q][j] >= e for every peer q; sum the W contributions in rank order
//            (deterministic), optimizer update of my chunk's slice, store the new parameters to
//            EVERY rank's parameter buffer (self included, write-through), drain, DONE_q[b][me][j] = e
//   final    (the step's last bucket, on the compute stream) wait DONE_me[b'][q][*] >= e for every
//            bucket, rank and slice: when the kernel ends, every parameter of this step has
//            landed and the next forward (a later kernel: L2 invalidated at its start) reads them.
// Buffer reuse is safe by construction: a rank overwrites an inbox slot (step e+1 backward) only
// after its step e+1 forward, i.e. after the final wait saw every owner's DONE of step e, which
// each owner sets after reading that slot; an owner writes a peer's parameters of bucket b only
// after that peer's ARRIVE for b, i.e. after its backward segment b, the last reader of them.
// Flags live in uncached device memory, each has ONE writer and is only stored (never
// read-modify-written) and polled, all with system-scope atomic loads/stores; payload
// stores carry sc0|sc1 (system write-through) and every storing wave drains (vmcnt(0)) before
// the workgroup barrier that precedes the flag store.  Every wait is bounded: on timeout the
// kernel records an error word in host memory and runs to completion (no GPU hang); the host
// raises at the next step.
#include <stdlib.h>
#include <string.h>

#include <stdexcept>
#include <string>

#include "api.h"
#include "common.h"
#include "xgmi_dev.h"

namespace ddl {

namespace {

// The READY gate ahead of this kernel timed out (its gradients may be incomplete): publish
// nothing, record error 6 (the peers' waits then time out as well and every host raises).
DDL_DEV bool gate_failed(const XgmiLaunch& a) {
  if (!a.gate_err || __hip_atomic_load(a.gate_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0)
    return false;
  if (threadIdx.x == 0) __hip_atomic_store(a.err, 6, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return true;
}

DDL_DEV float4 scale4(float4 x, float a) {
  x.x *= a; x.y *= a; x.z *= a; x.w *= a;
  return x;
}

// ---- debug checksums (DDL_XGMI_CHECK=1, the sync analogue of async --check-provenance) ------
// The pusher of slice j of bucket b stores, next to its ARRIVE word at the owner, the wrapping
// sum of the 32-bit patterns of exactly the floats it pushed; the owner recomputes that sum over
// what it reads from its inbox before it uses the slice and records error code 3 (and skips the
// update) on a mismatch — a stale or torn inbox read is caught where it happens, per (bucket,
// source, step), instead of as a parameter divergence steps later.
// The replicated bucket's checksum words carry the step parity like its inbox slots: a peer may
// publish step e+1's checksum (its parity-(e+1) slot) while this rank still checks step e's —
// with one word per (bucket, source, slice) the check of step e read step e+1's sum (error 3
// in the W = 8 one-card test, where ranks drift a whole step apart).  Owner buckets need no
// parity: a pusher writes an owner's inbox again only after that owner's DONE, i.e. after its
// check.
DDL_DEV int ck_idx(int b, int src, int j, int par = 0) {
  return (2 + par) * kXgmiMaxBuckets * kXgmiMaxPeers * kXgmiMaxSlices + xg_arrive_idx(b, src, j);
}

DDL_DEV uint32_t bits4(float4 v) {
  return __float_as_uint(v.x) + __float_as_uint(v.y) + __float_as_uint(v.z) + __float_as_uint(v.w);
}
// sum over the 256 threads of the workgroup (every thread gets it); red: 4 words of LDS
DDL_DEV uint32_t block_sum(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// ---- the steps of a slice's round, written once; the three kernels below compose them ---------

// Source q's piece of the slice in this rank's inbox: a descriptor and the byte offset of the
// piece's first float4.  Each kernel hands the steps its inbox addressing as a functor q -> Piece.
struct Piece {
  brsrc_t in;
  int off;
};
// What a workgroup knows of its round, read from the arguments once at the kernel's start (a
// value reloaded from them further down, past a divergent branch, would count as divergent and
// take the rank loops' addresses out of the scalar unit).
struct Round {
  int W, me, b, j;        // world size, this rank, the bucket, the slice
  long long deadline;     // of every wait of this launch
  uint32_t* myflags;
  uint32_t* red;          // LDS: block_sum's 4 words
  int* arrived;           // LDS: cleared when the wait or the check of the slice failed
};

// Every storing wave drains its write-through stores, the workgroup meets, and only then the
// chosen lanes store `epoch` into word `word` of rank dst's flags (xgmi_dev.h: why the drain is
// enough and no L2 write-back is needed).
DDL_DEV void publish(const XgmiTable& T, bool lane, int dst, int word, uint32_t epoch) {
  drain_vmem();
  __syncthreads();
  if (lane) xg_flag_store(T.flags[dst] + word, epoch);
}

// The ARRIVE wait: every peer's piece of slice j has arrived (one parallel poll, lane q for peer
// q).  *arrived (LDS) ends 0 if any wait failed (timeout, or another workgroup's recorded error).
DDL_DEV void wait_arrivals(const XgmiLaunch& a, const Round& g) {
  const int tid = threadIdx.x;
  if (tid == 0) *g.arrived = 1;
  __syncthreads();
  if (tid < g.W && tid != g.me &&
      !xg_wait_ge(g.myflags + xg_arrive_idx(g.b, tid, g.j), a.epoch, g.deadline, a.err, 1))
    *g.arrived = 0;  // benign race: every writer stores 0
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  // keep the loads below the poll
}

// Check mode: every peer's piece (n4 float4) against the checksum it published; a mismatch
// records error code 3 and clears *arrived.  par: the replicated bucket's step parity.
template <class P>
DDL_DEV void verify_pieces(const XgmiLaunch& a, const Round& g, int par, int n4, P piece) {
  if (!a.check || !*g.arrived) return;
  bool ok = true;
  for (int q = 0; q < g.W; ++q) {
    if (q == g.me) continue;
    const Piece p = piece(q);
    uint32_t c = 0;
    for (int i = threadIdx.x; i < n4; i += 256) c += bits4(bload4_sys(p.in, p.off + i * 16));
    const uint32_t got = block_sum(c, g.red);
    const uint32_t want = __hip_atomic_load(g.myflags + ck_idx(g.b, q, g.j, par), __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_SYSTEM);
    ok &= got == want;
  }
  if (!ok && threadIdx.x == 0) {
    __hip_atomic_store(a.err, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    *g.arrived = 0;
  }
  __syncthreads();
}

// Reduce and update the slice's n4 float4: parameters and own gradient at element `po` of this
// rank's buffers, optimizer state at element `so`, the peers' pieces through `piece`.  The W
// contributions (the own one scaled by coef, as the pushed ones were) are summed from zero in
// rank order: the same bits on every run, every rank and every rank count, and the RCCL reduce's.
// If the wait or the check failed the slice is NOT updated: summing a stale inbox would advance
// m / v and push wrong parameters into every replica.  The kernels still store DONE, so the peers
// do not wait out their own timeouts; the host raises on the error word.
// ALL: the new parameters go to every rank's copy, this one included, write-through, so a later
// kernel of any rank (other XCD, other GPU) reads them from memory even while this kernel is
// still running; workgroup j starts at a different rank.  Else to this rank's copy only (the
// next forward is a later kernel of this stream).
// NQ = world size when instantiated for it (loops over ranks fully unrolled: all of an element's
// remote loads / stores are in flight together), else kXgmiMaxPeers.
template <int NQ, bool ALL, class P>
DDL_DEV void reduce_update(const XgmiTable& T, const XgmiLaunch& a, const Round& g, P piece,
                           int64_t po, int64_t so, int n4) {
  const int W = g.W, me = g.me, j = g.j;
  const int n4u = *g.arrived ? n4 : 0;
  const float4* own = reinterpret_cast<const float4*>(a.grads + po);
  float4* m4 = a.m ? reinterpret_cast<float4*>(a.m + so) : nullptr;
  float4* v4 = a.v ? reinterpret_cast<float4*>(a.v + so) : nullptr;
  float4* w4 = reinterpret_cast<float4*>(T.params[me] + po);
  for (int i = threadIdx.x; i < n4u; i += 256) {
    float4 x[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q >= W) continue;
      if (q == me) {
        x[q] = a.coef != 1.f ? scale4(own[i], a.coef) : own[i];
      } else {
        const Piece p = piece(q);
        x[q] = bload4_sys(p.in, p.off + i * 16);
      }
    }
    float4 w = w4[i];
    float4 sum = f4zero();
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (q < W) { sum.x += x[q].x; sum.y += x[q].y; sum.z += x[q].z; sum.w += x[q].w; }
    upd4_any(a.rule, a.step, w, sum, m4, v4, i);
    if (ALL) {
#pragma unroll
      for (int k = 0; k < NQ; ++k)
        if (k < W)
          bstore4_sys(make_rsrc(T.params[(me + k + j) % W] + po, (uint32_t)n4 * 16u), i * 16, w);
    } else {
      w4[i] = w;
    }
  }
}

// WT = world size when instantiated for it, 0 = any world size (reduce_update's NQ).
template <int WT>
__global__ void __launch_bounds__(256) xgmi_ps_kernel(XgmiTable T, XgmiLaunch a) {
  if (gate_failed(a)) return;
  constexpr int NQ = WT ? WT : kXgmiMaxPeers;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int W = WT ? WT : a.world, me = a.rank, b = a.bucket;
  const long long deadline = wall_clock64() + a.timeout_ticks;
  const XgSlice s = xg_slice(j, a.slice, a.c);
  const int64_t s0 = s.s0;
  const int n4 = s.n4;
  const int64_t po = a.lo + me * a.c + s0;  // my chunk's slice in the plan buffer
  uint32_t* myflags = T.flags[me];
  __shared__ uint32_t red[4];
  __shared__ int arrived;
  const Round g{W, me, b, j, deadline, myflags, red, &arrived};

  // ---- phase 1: push my gradient pieces to their owners.  Per element index every owner's
  // load is issued before the first store; workgroup j starts at a different owner so the
  // W-1 links carry traffic at once.
  uint32_t cs[NQ - 1];
#pragma unroll
  for (int k = 0; k < NQ - 1; ++k) cs[k] = 0;
  for (int i = tid; i < n4; i += 256) {
    float4 x[NQ - 1];
#pragma unroll
    for (int k = 0; k < NQ - 1; ++k) {
      if (k < W - 1) {
        const int r = (me + 1 + (k + j) % (W - 1)) % W;
        x[k] = reinterpret_cast<const float4*>(a.grads + a.lo + r * a.c + s0)[i];
      }
    }
#pragma unroll
    for (int k = 0; k < NQ - 1; ++k) {
      if (k < W - 1) {
        const int r = (me + 1 + (k + j) % (W - 1)) % W;
        const brsrc_t dst = make_rsrc(T.inbox[r] + a.inbox_off + (int64_t)me * a.c + s0,
                                      (uint32_t)n4 * 16u);
        const float4 v = a.coef != 1.f ? scale4(x[k], a.coef) : x[k];
        bstore4_sys(dst, i * 16, v);
        if (a.check) cs[k] += bits4(v);
      }
    }
  }
  if (a.check) {  // publish each owner's checksum before the ARRIVE word (same drain covers it)
#pragma unroll
    for (int k = 0; k < NQ - 1; ++k) {
      if (k < W - 1) {
        const uint32_t t = block_sum(cs[k], red);
        const int r = (me + 1 + (k + j) % (W - 1)) % W;
        if (tid == 0)
          __hip_atomic_store(T.flags[r] + ck_idx(b, me, j), t, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
  publish(T, tid < W && tid != me, tid, xg_arrive_idx(b, me, j), a.epoch);

  // ---- phase 2: my chunk's slice, from every peer's slot [q] of my inbox, to every rank
  const brsrc_t inbox = make_rsrc(T.inbox[me] + a.inbox_off, (uint32_t)(W * a.c * 4));
  auto piece = [&](int q) { return Piece{inbox, (int)(((int64_t)q * a.c + s0) * 4)}; };
  wait_arrivals(a, g);
  verify_pieces(a, g, 0, n4, piece);
  reduce_update<NQ, true>(T, a, g, piece, po, s0, n4);
  publish(T, tid < W, tid, xg_done_idx(b, me, j), a.epoch);

  // ---- final wait: every bucket's new parameters from every owner have landed here
  if (a.final_wait) xg_final_wait(a, myflags, W, deadline);
}

// The step's LAST bucket, replicated: nothing overlaps its exchange — it is
// complete only after the final backward launch — so instead of push chunk -> owner update ->
// push parameters -> DONE (two cross-GPU hops on the critical path), every rank pushes the
// WHOLE bucket gradient to every peer (W-1 links at once, 208 KB each for conv1+conv2), sums the
// W contributions in rank order and runs the update itself on replicated optimizer state, then
// stores only its own parameters.  One hop, and no DONE words.  The inbox has two parity slots
// per source: a peer writes slot (e+1)&1 of step e+1 while this rank may still read slot e&1; it
// can write slot e&1 again only at step e+2, after its final wait of step e+1 saw this rank's
// DONE of every owner bucket at e+1 — issued after this rank's step-e+1 forward, i.e. after this
// kernel of step e.  This needs the replicated bucket to be the one the last backward segment
// completes (conv1 + conv2, launched on the compute stream): parallel/native_exchange.py
// last_segment_bucket.
template <int WT>
__global__ void __launch_bounds__(256) xgmi_repl_kernel(XgmiTable T, XgmiLaunch a) {
  if (gate_failed(a)) return;
  constexpr int NQ = WT ? WT : kXgmiMaxPeers;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int W = WT ? WT : a.world, me = a.rank, b = a.bucket;
  const long long deadline = wall_clock64() + a.timeout_ticks;
  const XgSlice s = xg_slice(j, a.slice, a.c);  // replicated: a.c is the whole bucket
  const int64_t s0 = s.s0;
  const int n4 = s.n4;
  const int par = (int)(a.epoch & 1u);
  uint32_t* myflags = T.flags[me];
  __shared__ uint32_t red[4];
  __shared__ int arrived;
  const Round g{W, me, b, j, deadline, myflags, red, &arrived};
  const float4* own = reinterpret_cast<const float4*>(a.grads + a.lo + s0);
  // slot (par, src) of rank r's replicated inbox, this slice
  auto slot = [&](int r, int src) {
    return make_rsrc(T.inbox[r] + a.inbox_off + ((int64_t)par * W + src) * a.rslot + s0,
                     (uint32_t)n4 * 16u);
  };

  // ---- phase 1: my whole slice to every peer
  uint32_t cs = 0;
  for (int i = tid; i < n4; i += 256) {
    float4 x = own[i];
    if (a.coef != 1.f) x = scale4(x, a.coef);
    if (a.check) cs += bits4(x);
#pragma unroll
    for (int k = 0; k < NQ - 1; ++k)
      if (k < W - 1) bstore4_sys(slot((me + 1 + (k + j) % (W - 1)) % W, me), i * 16, x);
  }
  if (a.check) {
    const uint32_t t = block_sum(cs, red);
    if (tid < W && tid != me)
      __hip_atomic_store(T.flags[tid] + ck_idx(b, me, j, par), t, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
  publish(T, tid < W && tid != me, tid, xg_arrive_idx(b, me, j), a.epoch);

  // ---- phase 2: the whole slice, from every peer's parity slot, to my copy
  auto piece = [&](int q) { return Piece{slot(me, q), 0}; };
  wait_arrivals(a, g);
  verify_pieces(a, g, par, n4, piece);
  reduce_update<NQ, false>(T, a, g, piece, a.lo + s0, s0, n4);
  if (a.final_wait) xg_final_wait(a, myflags, W, deadline);
}

// One OWNER bucket: a tensor-granular plan's exchange unit — the ranges of
// one PS's tensors that backward segment s completes — with a single owner, the rank hosting
// that PS (reference: every worker Sends the PS's tensors to it, the PS sums the W arrivals,
// applies Adam and Sends the parameters back, mnist_sync/parameter_server.py:52-69,
// mnist_sync_sharding/parameter_server.py:108-126).  Workgroup j owns slice j of the unit; a
// slice lies inside one run (plan-buffer range), so its gradient, parameters and optimizer state
// are each one contiguous span.
//   every rank but the owner: push my slice to the owner's inbox slot [me], drain, ARRIVE = e;
//   the owner: wait for every peer's ARRIVE, sum the W contributions in rank order, update with
//   the PS's state, store the parameters to EVERY rank (write-through), drain, DONE_q[owner] = e.
// A non-owner's workgroups end after their push (unless they carry the step's final wait), so an
// unbalanced plan (contiguous at W = 8: PS 7 owns 59 % of the bytes) loads only its owner's CUs
// and links.  Same flags, bounds, error words and reuse argument as xgmi_ps_kernel: a rank
// rewrites the owner's inbox slot only after its next forward, i.e. after its final wait saw the
// owner's DONE, which the owner sets after reading that slot.
template <int WT>
__global__ void __launch_bounds__(256) xgmi_owner_kernel(XgmiTable T, XgmiLaunch a) {
  if (gate_failed(a)) return;
  constexpr int NQ = WT ? WT : kXgmiMaxPeers;
  const int j = blockIdx.x, tid = threadIdx.x;
  const int W = WT ? WT : a.world, me = a.rank, b = a.bucket, own = a.owner;
  const long long deadline = wall_clock64() + a.timeout_ticks;
  int r = 0;
#pragma unroll
  for (int k = 1; k < kXgmiMaxRuns; ++k)
    if (k < a.nruns && j >= a.run_sl0[k]) r = k;
  const XgSlice s = xg_slice(j - a.run_sl0[r], a.run_slice[r], a.run_n[r]);
  const int n4 = s.n4;
  const int64_t lo = a.run_lo[r] + s.s0;    // plan-buffer offset of the slice
  const int64_t vo = a.run_voff[r] + s.s0;  // its offset in the unit's inbox slot
  uint32_t* myflags = T.flags[me];
  __shared__ uint32_t red[4];
  __shared__ int arrived;
  const Round g{W, me, b, j, deadline, myflags, red, &arrived};

  if (me != own) {
    const float4* mine = reinterpret_cast<const float4*>(a.grads + lo);
    const brsrc_t dst = make_rsrc(T.inbox[own] + a.inbox_off + (int64_t)me * a.c + vo,
                                  (uint32_t)n4 * 16u);
    uint32_t cs = 0;
    for (int i = tid; i < n4; i += 256) {
      const float4 x = mine[i];
      const float4 v = a.coef != 1.f ? scale4(x, a.coef) : x;
      bstore4_sys(dst, i * 16, v);
      if (a.check) cs += bits4(v);
    }
    if (a.check) {  // the slice's checksum at the owner, before the ARRIVE word (same drain)
      const uint32_t t = block_sum(cs, red);
      if (tid == 0)
        __hip_atomic_store(T.flags[own] + ck_idx(b, me, j), t, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    publish(T, tid == 0, own, xg_arrive_idx(b, me, j), a.epoch);
    if (a.final_wait) xg_final_wait(a, myflags, W, deadline);
    return;
  }

  // the owner: the unit's slice, from every peer's slot [q] of my inbox, to every rank
  const brsrc_t inbox = make_rsrc(T.inbox[me] + a.inbox_off, (uint32_t)(W * a.c * 4));
  auto piece = [&](int q) { return Piece{inbox, (int)(((int64_t)q * a.c + vo) * 4)}; };
  wait_arrivals(a, g);
  verify_pieces(a, g, 0, n4, piece);
  reduce_update<NQ, true>(T, a, g, piece, lo, a.run_soff[r] + s.s0, n4);
  publish(T, tid < W, tid, xg_done_idx(b, me, j), a.epoch);
  if (a.final_wait) xg_final_wait(a, myflags, W, deadline);
}

#define X_CHECK(x)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess)                                                                 \
      throw std::runtime_error(std::string("xgmi: ") + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

struct HandleBlob {  // what one rank publishes (exchanged as bytes over the default group)
  hipIpcMemHandle_t params, inbox, flags;
  int64_t params_off;
  int32_t world, rank;
};

}  // namespace

// ---- PeerMap: the exported buffers and their mappings (PeerExchange, AsyncPeer) -----------------
#define MAP_CHECK(x)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess)                                                               \
      throw std::runtime_error(std::string(tag_) + ": " + #x + ": " + hipGetErrorString(e_)); \
  } while (0)

PeerMap::PeerMap(const char* tag, float* params, int world, int rank, double default_timeout_s)
    : tag_(tag), params_(params), world_(world), rank_(rank) {
  timeout_s = xgmi_timeout_s(default_timeout_s);  // a healthy wait takes microseconds
}

void PeerMap::alloc(int64_t inbox_elems, size_t flag_bytes) {
  MAP_CHECK(hipMalloc(&my_inbox, inbox_elems * sizeof(float)));
  MAP_CHECK(hipMemset(my_inbox, 0, inbox_elems * sizeof(float)));
  MAP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&my_flags), flag_bytes,
                                  hipDeviceMallocUncached));
  MAP_CHECK(hipMemset(my_flags, 0, flag_bytes));
  MAP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&err), 64, hipHostMallocDefault));
  memset(err, 0, 64);
}

void PeerMap::unmap_peers() {
  if (opened) (void)hipDeviceSynchronize();
  for (int q = 0; q < world_; ++q) {
    if (q == rank_) continue;
    for (void*& p : mapped_[q]) {
      if (p) (void)hipIpcCloseMemHandle(p);
      p = nullptr;
    }
  }
  opened = false;
}

void PeerMap::close() {
  if (my_inbox || my_flags || opened) (void)hipDeviceSynchronize();
  unmap_peers();
  if (my_inbox) (void)hipFree(my_inbox);
  if (my_flags) (void)hipFree(my_flags);
  if (err) (void)hipHostFree(err);
  my_inbox = nullptr;
  my_flags = nullptr;
  err = nullptr;
}

std::string PeerMap::handle() const {
  HandleBlob h;
  memset(&h, 0, sizeof(h));
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  MAP_CHECK(hipMemGetAddressRange(&base, &size, params_));
  MAP_CHECK(hipIpcGetMemHandle(&h.params, base));
  h.params_off = reinterpret_cast<const char*>(params_) - reinterpret_cast<const char*>(base);
  MAP_CHECK(hipIpcGetMemHandle(&h.inbox, my_inbox));
  MAP_CHECK(hipIpcGetMemHandle(&h.flags, my_flags));
  h.world = world_;
  h.rank = rank_;
  return std::string(reinterpret_cast<const char*>(&h), sizeof(h));
}

void PeerMap::open(const std::vector<std::string>& handles) {
  const std::string tag(tag_);
  if ((int)handles.size() != world_) throw std::invalid_argument(tag + ": one handle per rank");
  for (int q = 0; q < world_; ++q) {
    if (handles[q].size() != sizeof(HandleBlob)) throw std::invalid_argument(tag + ": bad handle");
    HandleBlob h;
    memcpy(&h, handles[q].data(), sizeof(h));
    if (h.world != world_ || h.rank != q) throw std::invalid_argument(tag + ": handle rank");
    if (q == rank_) {
      table.params[q] = params_;
      table.inbox[q] = my_inbox;
      table.flags[q] = my_flags;
      continue;
    }
    void *p = nullptr, *ib = nullptr, *fl = nullptr;
    MAP_CHECK(hipIpcOpenMemHandle(&p, h.params, hipIpcMemLazyEnablePeerAccess));
    mapped_[q][0] = p;
    MAP_CHECK(hipIpcOpenMemHandle(&ib, h.inbox, hipIpcMemLazyEnablePeerAccess));
    mapped_[q][1] = ib;
    MAP_CHECK(hipIpcOpenMemHandle(&fl, h.flags, hipIpcMemLazyEnablePeerAccess));
    mapped_[q][2] = fl;
    table.params[q] = reinterpret_cast<float*>(reinterpret_cast<char*>(p) + h.params_off);
    table.inbox[q] = reinterpret_cast<float*>(ib);
    table.flags[q] = reinterpret_cast<uint32_t*>(fl);
  }
  opened = true;
}
#undef MAP_CHECK

static std::vector<XgmiBucketSpec> equal_specs(
    const std::vector<std::pair<int64_t, int64_t>>& buckets) {
  std::vector<XgmiBucketSpec> v;
  for (const auto& b : buckets) {
    XgmiBucketSpec s;
    s.runs.push_back(b);
    v.push_back(s);
  }
  return v;
}

PeerExchange::PeerExchange(float* params, const float* grads, int64_t total, int world, int rank,
                           const std::vector<std::pair<int64_t, int64_t>>& buckets, int max_slices,
                           int repl_bucket)
    : PeerExchange(params, grads, total, world, rank, equal_specs(buckets), max_slices,
                   repl_bucket) {}

PeerExchange::PeerExchange(float* params, const float* grads, int64_t total, int world, int rank,
                           const std::vector<XgmiBucketSpec>& buckets, int max_slices,
                           int repl_bucket)
    : repl_(repl_bucket), params_(params), grads_(grads), total_(total), world_(world),
      rank_(rank), map_("xgmi", params, world, rank, 20.0) {
  if (reinterpret_cast<uintptr_t>(params) % 16 || reinterpret_cast<uintptr_t>(grads) % 16)
    throw std::invalid_argument("xgmi: buffers must be 16-B aligned");
  init(buckets, max_slices);
}

// The plan (xgmi_plan.h: refusals, slices, inbox offsets), then what needs HIP.  The records are
// finished last: the error word exists only after alloc.
void PeerExchange::init(const std::vector<XgmiBucketSpec>& buckets, int max_slices) {
  XgmiPlan plan = plan_buckets(buckets, total_, world_, rank_, max_slices, repl_);
  // ARRIVE, DONE and (check mode) checksum words, the replicated bucket's in two parities
  map_.alloc(plan.inbox, 4ull * kXgmiMaxBuckets * kXgmiMaxPeers * kXgmiMaxSlices * sizeof(uint32_t));
  X_CHECK(hipDeviceSynchronize());
  check_ = env_flag("DDL_XGMI_CHECK", false, /*only_1=*/true);
  bk_ = std::move(plan.rec);
  for (XgmiLaunch& a : bk_) {
    a.grads = grads_;
    a.err = map_.err;
    a.timeout_ticks = map_.timeout_ticks();
    a.check = check_ ? 1 : 0;
  }
}

PeerExchange::~PeerExchange() { close(); }

void PeerExchange::fill(int bucket, uint32_t epoch, const XgmiUpdate& u, bool final_wait,
                        bool gated, XgmiLaunch& a) const {
  if (!map_.opened) throw std::runtime_error("xgmi: open() the peer handles first");
  if (bucket < 0 || bucket >= (int)bk_.size()) throw std::invalid_argument("xgmi: bucket index");
  const bool owns = owner(bucket) < 0 || owner(bucket) == rank_;  // runs (part of) the update
  if (owns && u.rule.kind != kUpdCopy && !u.m)
    throw std::invalid_argument("xgmi: optimizer state missing");
  if (owns && u.rule.kind == kUpdAdam && !u.v) throw std::invalid_argument("xgmi: Adam needs v");
  a = bk_[bucket];
  a.final_wait = final_wait ? 1 : 0;
  a.epoch = epoch;
  a.m = u.m;
  a.v = u.v;
  a.rule = u.rule;
  a.step = u.step;
  a.coef = u.coef;
  a.gate_err = gated ? gate_err_ : nullptr;
}

// The kernel of a bucket family (0 owner, 1 replicated, 2 equal-chunk) with its rank loops
// unrolled for world size N (0: any).  Only the owner family has a <1> form.
using XgmiKernel = void (*)(XgmiTable, XgmiLaunch);
template <int N>
static XgmiKernel bucket_kernel(int family) {
  constexpr int M = N == 1 ? 0 : N;
  return family == 0 ? xgmi_owner_kernel<N> : family == 1 ? xgmi_repl_kernel<M> : xgmi_ps_kernel<M>;
}

void PeerExchange::launch(int bucket, uint32_t epoch, const XgmiUpdate& u, bool final_wait,
                          hipStream_t st, bool gated) {
  XgmiLaunch a;
  fill(bucket, epoch, u, final_wait, gated, a);
  const int family = owner(bucket) >= 0 ? 0 : bucket == repl_ ? 1 : 2;
  XgmiKernel k = bucket_kernel<0>(family);
  switch (world_) {
#define X_CASE(N) case N: k = bucket_kernel<N>(family); break;
    X_CASE(1) X_CASE(2) X_CASE(3) X_CASE(4) X_CASE(5) X_CASE(6) X_CASE(7) X_CASE(8)
#undef X_CASE
  }
  DDL_LAUNCH(k, dim3(nslices(bucket)), dim3(256), 0, st, map_.table, a);
  DDL_CHECK_LAUNCH();
}

// ---- the stale-L2 probe of the xGMI self-test (native_exchange.py) ----------------------------
// A peer's parameter stores reach this GPU's HBM over xGMI without touching its eight per-XCD
// L2s, so a line that some XCD cached BEFORE the exchange could be read back stale by the next
// kernel unless that kernel's start acquire invalidates it (the protocol's assumption, header
// comment above).  The probe makes the hazard reachable on purpose: the sweep is launched with 8
// blocks per 16 KB chunk, block b on XCD b % 8 (the hardware's round-robin dispatch), so before
// the exchange every XCD reads — and caches, with ordinary loads — every line of the buffer, and
// after it every XCD compares every line with the expected values.  want == null: warm only.
__global__ void __launch_bounds__(256) xcd_sweep_kernel(const float4* __restrict__ a,
                                                        const float4* __restrict__ want,
                                                        int64_t n4, int* __restrict__ out) {
  const int64_t chunk = blockIdx.x >> 3;
  const int64_t lo = chunk * 1024, hi = lo + 1024 < n4 ? lo + 1024 : n4;
  int bad = 0;
  float acc = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float4 v = a[i];
    if (want) {
      const float4 w = want[i];
      bad += (v.x != w.x) + (v.y != w.y) + (v.z != w.z) + (v.w != w.w);
    } else {
      acc += v.x + v.y + v.z + v.w;
    }
  }
  if (bad) atomicAdd(out, bad);
  if (!want && acc == 1.2345e-30f) atomicAdd(out + 1, 1);  // keeps the warm loads alive
}

void launch_xcd_sweep(const float* a, const float* want, int64_t n, int* out, hipStream_t st) {
  if (n % 4 || reinterpret_cast<uintptr_t>(a) % 16 || (want && reinterpret_cast<uintptr_t>(want) % 16))
    throw std::invalid_argument("xcd sweep: 16-B aligned float4 buffers");
  const int64_t n4 = n / 4, chunks = (n4 + 1023) / 1024;
  if (chunks <= 0) return;
  DDL_LAUNCH(xcd_sweep_kernel, dim3((unsigned)(chunks * 8)), dim3(256), 0, st,
             reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(want), n4, out);
}

}  // namespace ddl
