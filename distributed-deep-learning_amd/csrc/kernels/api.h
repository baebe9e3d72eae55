// Host-side launch API of the gfx950 kernels (raw device pointers + hipStream_t; no torch).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "clip_ranges.h"
#include "ps_bank.h"
#include "runtime/session.h"
#include "schedule.h"
#include "scratch.h"
#include "tail.h"
#include "xgmi_plan.h"

namespace ddl {

class ShmMailbox;

// A boolean DDL_* environment variable: `def` when unset; when set, off only for a leading '0'
// (only_1: on only for a leading '1')
inline bool env_flag(const char* name, bool def, bool only_1 = false) {
  const char* e = getenv(name);
  return !e ? def : only_1 ? e[0] == '1' : e[0] != '0';
}
// DDL_XGMI_TIMEOUT_S: the bound of every xGMI wait and of the runner's READY gate, in seconds
inline double xgmi_timeout_s(double def) {
  const char* e = getenv("DDL_XGMI_TIMEOUT_S");
  return e ? atof(e) : def;
}

// ---- optimizer (optim.hip) -------------------------------------------------------------------
// One update of span s from gradient g under rule r (update.h) with step size `step`: the 16-B
// vector kernel when every stream the rule has is 16-B aligned, else the scalar one (the same
// bits).  Every stand-alone optimizer launch of the runtime goes through here.
void launch_update(const UpdRule& r, float step, const UpdSpan& s, const float* g, int64_t n,
                   hipStream_t st, int max_grid = 2048);
void launch_scale(float* p, int64_t n, float a, hipStream_t st);

// ---- clip by global norm (clip.hip) ----------------------------------------------------------
// norm over the ranges of g (clip_ranges.h), coef = max_norm / norm when norm > max_norm else 1
// (also when the norm is not finite), g *= coef in place unless coef == 1.  out2: {norm, coef}
// on the device; partials: t.nchunks doubles; ticket: one zeroed int (left zero).  Two launches,
// no host sync; the bits depend on (contents, ranges, max_norm) only, not on max_grid.
void launch_clip(const ClipRanges& t, float* g, float max_norm, float* out2, double* partials,
                 int* ticket, hipStream_t st, int max_grid = 0);
// one clipping site of a step runner (set_clip): the table and the caller's device scratch
struct ClipSite {
  ClipRanges ranges;
  float max_norm = 0.f;          // 0: off
  float* out2 = nullptr;
  double* partials = nullptr;
  int* ticket = nullptr;
  bool on() const { return max_norm > 0.f; }
  void launch(float* g, hipStream_t st) const {
    launch_clip(ranges, g, max_norm, out2, partials, ticket, st);
  }
};

// ---- gradient accumulation over K micro-batches (accum.hip) ---------------------------------
// over the ranges of g and of the accumulator acc (same size, same 16-byte alignment):
//   kAccumFirst  acc := g (bits copied)      kAccumAdd  acc := acc + g
//   kAccumFinish g := (acc + g) * (float)(1.0 / k)
// One launch, no host sync; the bits do not depend on max_grid.
enum { kAccumFirst = 0, kAccumAdd = 1, kAccumFinish = 2 };
void launch_accum(const ClipRanges& t, float* g, float* acc, int mode, int k, hipStream_t st,
                  int max_grid = 0);
// one accumulation site of a step runner (set_accum): the table, K, the caller's accumulator and
// the micro-batches accumulated so far in the open step
struct AccumSite {
  ClipRanges ranges;
  int k = 1;                     // 1: off
  float* acc = nullptr;
  int done = 0;
  bool on() const { return k > 1; }
  // a non-final micro-batch's gradient is in g
  void accumulate(float* g, hipStream_t st) {
    launch_accum(ranges, g, acc, done == 0 ? kAccumFirst : kAccumAdd, k, st);
    ++done;
  }
  // the final micro-batch's gradient is in g: g <- the mean over the K micro-batches
  void finish(float* g, hipStream_t st) {
    launch_accum(ranges, g, acc, kAccumFinish, k, st);
    done = 0;
  }
  // refuse a micro-batch out of turn (`final`: the step's last)
  void expect(bool final) const {
    if (!on()) {
      if (!final) throw std::invalid_argument("accumulate(): no accumulation set (set_accum)");
      return;
    }
    if (final ? done != k - 1 : done >= k - 1)
      throw std::invalid_argument("accumulation: a step is K - 1 accumulate() calls, then step()");
  }
};

// what a step runner does to its worker's whole gradient before anything consumes it
struct GradStage {
  ClipSite clip;
  AccumSite accum;
  // the backward runs whole, nothing riding in it (an accumulated step's final micro-batch runs
  // as a clipped step does)
  bool whole() const { return clip.on() || accum.on(); }
  void finish(float* g, hipStream_t st) {  // the mean over the K micro-batches, then the clip
    if (accum.on()) accum.finish(g, st);
    if (clip.on()) clip.launch(g, st);
  }
};

// ---- shuffled, shift-augmented batches (batch.hip) ------------------------------------------
// rows [0, B) of xb [>= B,784] and yb [>= B] from the n training rows: row i is training row
// perm(base + i; n, key) (base + i unshuffled) translated by the draw of (base + i, key_shift) in
// [-s, s]^2, zero-filled (batch.h; ops/shuffle.py is the CPU twin).  base + B <= n; x_train and
// xb 16-byte aligned and apart.  One launch, no host sync.
void launch_assemble_batch(const float* x_train, const int64_t* y_train, int64_t n, float* xb,
                           int64_t* yb, int B, int64_t base, uint32_t key, uint32_t key_shift,
                           int s, bool shuffle, hipStream_t st);

// ---- conv1 forward as a direct LDS-staged kernel (conv1.hip) --------------------------------
// x [B,784], w [25,32], bias [32] -> pooled p1 [B,18,18,32] (halo layout) + codes [B,14,14,32]
void launch_conv1_fwd(const float* x, const float* w, const float* bias, float* out,
                      uint8_t* code, int B, hipStream_t st);
// conv1's weight / bias gradient, direct kernel with in-launch reduce (conv1.h); part /
// tickets: c1w_scratch_floats(B) floats and c1w_groups(B) + 1 zeroed ints of scratch
void launch_conv1_wgrad_only(const float* x, const float* d1, int B, float* gw, float* gb,
                             float* part, int* tickets, hipStream_t st);
bool conv1_wgrad_fits(int B, size_t slab_floats, int max_tickets);

// ---- classifier head (head.hip) --------------------------------------------------------------
void launch_head_fwd(const float* h2, const float* w, const float* bias, const int64_t* labels,
                     int B, float* dlog, float* loss, int* correct, hipStream_t st);
// fused head: logits, loss, dlogits and dh2 (with fc2's dropout backward) per sample; fc3's
// weight gradient is left to launch_head_wgrad or the next dual launch (head.h)
void launch_head_fused(const float* h2, const float* w, const float* bias, const int64_t* labels,
                       int B, const uint32_t* seed, uint32_t seed_v, uint32_t thr24,
                       float inv_keep, float* dlog, float* loss, float* dpre2, hipStream_t st);
void launch_head_wgrad(const float* h2, const float* dlog, int B, float* gw, float* gb,
                       hipStream_t st);
// launch_head_fused that first finishes fc2's forward: h2 = dropout(sum of the S split-K
// partials of fc2's one-wave 32x32 tiles + b2) per sample, stored for fc3's weight gradient
void launch_head_fused_fc2(const float* slab, int S, int gx, int ntiles, const float* b2,
                           float* h2, const float* w, const float* bias, const int64_t* labels,
                           int B, const uint32_t* seed, uint32_t seed_v, uint32_t thr24,
                           float inv_keep, float* dlog, float* loss, float* dpre2,
                           hipStream_t st);
void launch_head_bwd(const float* h2, const float* w, const float* dlog, int B,
                     const uint32_t* seed, uint32_t seed_v, uint32_t thr24, float inv_keep,
                     float* gw, float* gb, float* dpre2, hipStream_t st);

// ---- diagnostics (diag.hip) -------------------------------------------------------------------
void launch_mfma_peak(float* out, int blocks, int iters, hipStream_t st, int kind = 0);
void launch_gemm_nomem(float* out, int M, int N, int K, int splits, void* slab, int* tickets,
                       hipStream_t st);

// ---- the CNN step engine (engine.hip; its ops, configs and launch decisions: schedule.h) ------
struct Engine {
  // ---- the schedule (input): the tuned defaults with the DDL_* overrides on top
  Schedule sched;
  uint32_t thr24 = 0;        // dropout threshold (train)
  uint32_t seed_value = 0;   // dropout seed used when a step is given no device seed word
  float inv_keep = 1.f;

  // ---- the pending hand-offs: work one launch leaves to the next
  // optimizer tail (tail.h) for the next dual launch; consumed (and cleared) by it, or by
  // flush_tail() as a launch of its own when no dual launch takes it
  UpdTail tail;
  // the LAST segment's update (W = 1 tail path): conv1's part applied by its weight-gradient
  // reduce epilogue, the rest as tail blocks of that launch (engine_impl.h dual_then_b).
  // Cleared when taken; the runner launches it as before when it is still pending.
  UpdTail final_upd;
  // fc3 weight gradient still to compute (fused head kernel ran): taken by the fc2 dual launch
  int head_wgrad_pending = 0;
  // fc weight gradients the packed launches left to the conv4 dual launch (bit 0: fc2, 1: fc1)
  int fc_wgrad_pending = 0;
  // fc2 forward's split-K partials left to the head kernel (fc2_in_head); null: h2 is final
  const float* fc2_slab = nullptr;
  int fc2_S = 0, fc2_gx = 0, fc2_ntiles = 0;
  // the pending tail, handed to the launch that carries it
  UpdTail take_tail() {
    const UpdTail t = tail;
    if (t.nblocks > 0) hit(BR_TAIL_CONSUMED);
    tail = UpdTail();
    return t;
  }
  // stand-alone optimizer launches flush_tail() has issued for update tails no launch took
  // (host counter, diagnostic: SyncRunner::update_launches)
  int update_launches = 0;
  // host counters of the dispatch branches taken since the last reset (enum Branch)
  int branch_hits[BR_COUNT] = {};
  void hit(Branch b) { ++branch_hits[b]; }

  // ---- the buffers
  const float* P[14] = {};   // parameter tensors v0..v13 (any flat layout)
  float* G[14] = {};         // gradient tensors v0..v13
  int max_batch = 0;         // activation buffers sized for this batch
  int train_batch = 0;       // slab sized for this batch with the current splits/cfgs
  // workspace carve-out
  float *p1 = nullptr, *p2 = nullptr, *p3 = nullptr, *p4 = nullptr, *h1 = nullptr, *h2 = nullptr;
  float *dlog = nullptr, *loss = nullptr, *dpre2fc = nullptr, *dpre1fc = nullptr;
  float *d4 = nullptr, *d3 = nullptr, *d2 = nullptr, *d1 = nullptr;
  uint8_t *c1 = nullptr, *c2 = nullptr, *c3 = nullptr, *c4 = nullptr;
  int* correct = nullptr;
  size_t slab_floats = 0;
  SplitScratch scratch[2];   // [0] main stream, [1] weight-gradient stream
  static constexpr int kMaxTickets = 8192;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;

  Engine();
  ~Engine();
  void init_streams();
  // M, N, K of op `op` at batch B (used for slab sizing and by tests)
  static void op_shape(int op, int B, int* M, int* N, int* K);
  size_t slab_floats_needed(int B) const;
  size_t workspace_bytes() const;
  void bind_workspace(void* base);

  // forward through fc2 (train: dropout on, configured split-K; eval: no dropout, no split).
  // defer_fc2: the caller runs backward_segment(0) next, so fc2's wide reduce may be left to
  // the head kernel (fc2_in_head); otherwise h2 is final when forward returns
  void forward(const float* x, int B, const uint32_t* seed, bool train, hipStream_t st,
               bool defer_fc2 = false);
  // launch fc2's pending reduce on its own (no-op when none is pending)
  void flush_fc2(const uint32_t* seed, int B, hipStream_t st);
  // backward segment s (0: head+fc, 1: conv4, 2: conv3, 3: conv2+conv1); weight-gradient
  // GEMMs fork onto the side stream and join back at the end of the segment
  void backward_segment(int s, const float* x, const int64_t* labels, int B,
                        const uint32_t* seed, hipStream_t st);
  // eval: forward(train=false) + correct-count accumulation into *correct
  void eval_count(const float* x, const int64_t* labels, int B, hipStream_t st);
  // run a single GEMM op on `st` with scratch `si` (tests / tuning)
  void run_op(int op, const float* x, int B, const uint32_t* seed, bool train, hipStream_t st,
              int si = 0);
  // launch a pending optimizer tail on its own (no-op when none is pending)
  void flush_tail(hipStream_t st);
  void flush_head_wgrad(int B, hipStream_t st);
  // launch pending fc weight gradients on their own (no-op when none are pending)
  void flush_fc_wgrad(const float* x, int B, const uint32_t* seed, hipStream_t st);

 private:
  void fork(hipStream_t st);
  void join(hipStream_t st);
  void wgrad(int op, const float* x, int B, const uint32_t* seed, hipStream_t st);
};

// ---- what the two step runners share (runner.hip) -------------------------------------------
struct MicroBatch {  // on stream st; bwd_range: the trace range name of each backward segment
  const float* x;
  const int64_t* labels;
  int B;
  hipStream_t st;
  const char* const* bwd_range;
};
// the step's forward (fc2's reduce left to the head: the backward follows)
void run_forward(Engine& eng, const MicroBatch& mb);
// the four backward segments with nothing riding in them, then a pending tail flushed
void run_whole_backward(Engine& eng, const MicroBatch& mb);

struct LocalUpdates {     // one worker, every update local (W = 1)
  const UpdatePlan* plan;
  const OptimSpec* opt;   // the rule, and the momentum rule's step size
  const float* lr_t;      // the Adam rule's, by PS
  float* w;
  const float* g;
  int max_grid = 2048;    // of a stand-alone launch
  float step(const PlanPiece& p) const { return opt->step_for(lr_t[p.ps]); }
};
// launch_update of each piece; returns the launches issued
int launch_piece_updates(const LocalUpdates& u, const std::vector<PlanPiece>& pieces,
                         hipStream_t st);
struct RidePolicy {
  bool rides[kPlanSegments];  // the segment is offered as a tail; else launched piece by piece
  int first, f4_per_block;    // UpdTail's, of a tail beside a dual launch
  bool final_in_reduce;       // offer the last segment to conv1's weight-gradient launch
};
// The four backward segments with segment s - 1's update as the tail of segment s's launch
// (flushed as a launch of its own if the segment had no launch to take it) and the last segment's
// inside conv1's weight-gradient launch when the engine takes it (engine_impl.h dual_then_b),
// else launched after the backward.  Returns the stand-alone launches it issued itself (the
// engine counts flushed tails: Engine::update_launches).
int run_riding_backward(Engine& eng, const MicroBatch& mb, const LocalUpdates& u,
                        const RidePolicy& pol);

// May a wait for a kernel of stream `st` sit on stream `waiter` (null: any stream of the
// device's greatest priority)?  Only when the two cannot share a hardware queue: HIP pools
// hardware queues per priority, so when their priorities differ.  Queried once per `st`.
struct WaitPlacement {
  hipStream_t st = nullptr;
  bool checked = false, ok = false;
  bool safe(hipStream_t s, hipStream_t waiter) {
    if (checked && s == st) return ok;
    int lo = 0, hi = 0, p = 0, wp = 0;  // (the null stream is a normal-priority stream)
    ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
         (s == nullptr || hipStreamGetPriority(s, &p) == hipSuccess) &&
         (waiter == nullptr || hipStreamGetPriority(waiter, &wp) == hipSuccess) && hi != lo &&
         p != (waiter ? wp : hi);
    st = s;
    checked = true;
    return ok;
  }
};

// ---- native synchronous step runner (runner.hip) -------------------------------------------
struct RunnerRange {
  int64_t lo, hi;       // plan-buffer element range [lo, hi)
  int64_t state_off;    // offset of the range's optimizer state in the unit's m / v
};
struct RunnerUnit {
  // AR: all-reduce + update on replicated state (the last bucket); XGMI_REPL: its xGMI form
  enum Kind { LOCAL = 0, RS = 1, REDUCE = 2, XGMI = 3, AR = 4, XGMI_REPL = 5 };
  int seg = 0;          // backward segment after which the unit's gradients are complete
  int kind = LOCAL;
  int host = 0;         // REDUCE: rank that owns the PS
  int ps = 0;           // index into the per-step lr_t table (RS: this rank's PS)
  std::vector<RunnerRange> ranges;
  float* m = nullptr;   // optimizer state base of the owning PS (null where not hosted)
  float* v = nullptr;
  float* shard = nullptr;  // RS: 1/W chunk buffer
  int bucket = -1;         // XGMI: bucket index of the runner's PeerExchange
};

// ---- parameter-server exchange over xGMI peer memory (xgmi.hip) ------------------------------
// The limits, XgmiLaunch, XgmiBucketSpec and the slice and inbox plan: xgmi_plan.h.
struct XgmiTable {               // every rank's IPC-mapped buffers, indexed by rank
  float* params[kXgmiMaxPeers];
  float* inbox[kXgmiMaxPeers];
  uint32_t* flags[kXgmiMaxPeers];
};
struct XgmiUpdate {              // owner-side update of one bucket chunk
  UpdRule rule;                  // update.h (kUpdCopy: the self-test, w := summed g)
  float step = 0.f;              // Adam: lr_t of the owning PS; momentum: the learning rate
  float* m = nullptr;            // optimizer state of this rank's chunk of the bucket
  float* v = nullptr;
  float coef = 1.f;
};

// This rank's exported buffers and every rank's mapping of them: what PeerExchange and AsyncPeer
// both own (xgmi.hip).  `tag` prefixes its error messages.
class PeerMap {
 public:
  PeerMap(const char* tag, float* params, int world, int rank, double default_timeout_s);
  // the zeroed inbox and uncached flag words, the host error word; the caller synchronizes
  void alloc(int64_t inbox_elems, size_t flag_bytes);
  std::string handle() const;                         // this rank's IPC handles, as bytes
  void open(const std::vector<std::string>& handles);  // every rank's, in rank order
  // unmap the peers' buffers (after the device has drained).  HIP leaves freeing an exported
  // buffer undefined while a peer still has it mapped, so a process that goes on to build another
  // exchange lets every rank unmap first: unmap_peers(), a host barrier, close().
  void unmap_peers();
  void close();  // drain the device, unmap, free the inbox, the flags and the error word; idempotent
  int error() const { return err ? __atomic_load_n(err, __ATOMIC_ACQUIRE) : 0; }
  long long timeout_ticks() const { return (long long)(timeout_s * 1e8); }  // wall_clock64: 100 MHz

  XgmiTable table{};  // every rank's buffers, by rank (after open())
  float* my_inbox = nullptr;
  uint32_t* my_flags = nullptr;
  int* err = nullptr;
  double timeout_s;   // DDL_XGMI_TIMEOUT_S
  bool opened = false;

 private:
  const char* tag_;
  float* params_;
  int world_, rank_;
  void* mapped_[kXgmiMaxPeers][3] = {};
};

// The xGMI self-test's stale-L2 probe (xgmi.hip): every XCD reads every line of `a` (want null:
// warms the eight L2s) or counts into out[0] the elements that differ from `want`
void launch_xcd_sweep(const float* a, const float* want, int64_t n, int* out, hipStream_t st);

class PeerExchange {
 public:
  // buckets: [lo, hi) ranges of the flat plan buffer, each divisible by 4 * world; rank r owns
  // chunk r of every bucket.  Allocates the inbox (one slot per source rank) and the flags.
  // repl_bucket >= 0: that bucket is exchanged all-to-all and updated on every rank with
  // replicated optimizer state (xgmi_repl_kernel), instead of by its chunk owners
  PeerExchange(float* params, const float* grads, int64_t total, int world, int rank,
               const std::vector<std::pair<int64_t, int64_t>>& buckets, int max_slices,
               int repl_bucket = -1);
  // general form: equal-chunk and owner buckets (XgmiBucketSpec)
  PeerExchange(float* params, const float* grads, int64_t total, int world, int rank,
               const std::vector<XgmiBucketSpec>& buckets, int max_slices, int repl_bucket = -1);
  ~PeerExchange();
  // the fused push / owner update / pull of one bucket at step `epoch` (same on all ranks)
  // gated: the launch sits behind the runner's READY gate on the comm stream (checks its error
  // word before publishing anything)
  void launch(int bucket, uint32_t epoch, const XgmiUpdate& u, bool final_wait, hipStream_t st,
              bool gated = false);
  int error() const { return map_.error(); }  // nonzero once a wait timed out (1 arrive, 2 done)
  // the runner's READY-gate error word, checked by every bucket kernel before it publishes
  void set_gate_error(const int* w) { gate_err_ = w; }
  // unmap the peers' buffers and free this rank's (after the device has drained); idempotent
  void close() { map_.close(); }
  // the first half of close() alone (PeerMap::unmap_peers).  Nothing can be launched after it.
  void unmap_peers() { map_.unmap_peers(); }
  std::string handle() const { return map_.handle(); }
  void open(const std::vector<std::string>& handles) { map_.open(handles); }
  double timeout_s() const { return map_.timeout_s; }
  int num_buckets() const { return (int)bk_.size(); }
  int nslices(int b) const { return bk_[b].nslices[b]; }
  int64_t chunk(int b) const { return bk_[b].c; }
  int owner(int b) const { return bk_[b].owners[b]; }
  // elements of optimizer state a launch of bucket b may touch: [0, state_extent(b)) of m and v
  int64_t state_extent(int b) const {
    const XgmiLaunch& B = bk_[b];
    int64_t n = owner(b) >= 0 ? 0 : B.c;
    for (int r = 0; r < B.nruns; ++r)
      if (B.run_soff[r] + B.run_n[r] > n) n = B.run_soff[r] + B.run_n[r];
    return n;
  }
  int world() const { return world_; }
  int repl_bucket() const { return repl_; }
  bool check_mode() const { return check_; }

 private:
  void init(const std::vector<XgmiBucketSpec>& buckets, int max_slices);
  void fill(int bucket, uint32_t epoch, const XgmiUpdate& u, bool final_wait, bool gated,
            XgmiLaunch& a) const;
  int repl_ = -1;
  bool check_ = false;
  float* params_;
  const float* grads_;
  int64_t total_;
  int world_, rank_;
  // each bucket's launch record, every field set but the per-launch ones (fill)
  std::vector<XgmiLaunch> bk_;
  PeerMap map_;
  const int* gate_err_ = nullptr;
};

// ---- asynchronous PS over xGMI peer memory (xgmi_async.hip) ----------------------------------
// a rank's uncached device flags: its DONE words as a worker (dense over all PS' slices)
constexpr int kAsyncDense = kAsyncMaxPs * kAsyncMaxSlices;
constexpr size_t kAsyncFlagWords = (size_t)kAsyncDense;
struct AsyncTable {
  float* params[kXgmiMaxPeers];  // every rank's worker parameter buffer (IPC-mapped)
  float* inbox[kXgmiMaxPeers];
  uint32_t* flags[kXgmiMaxPeers];
  uint32_t* done;                // DONE[worker][ps][slice] in host memory shared by all ranks
  uint32_t* posted;              // the arrival board POSTED[ps][worker][slice], same segment
  // this rank's gradient buffer: with `elide` set, a push to a PS this rank hosts itself only
  // posts its words, and the apply of this worker's push reads the gradient here instead of an
  // inbox copy (the worker overwrites it only after its pull gate, i.e. after that apply)
  const float* grads;
  int elide;
  AsyncShard shard[kAsyncMaxPs];
};

class AsyncPeer {
 public:
  AsyncPeer(float* params, const float* grads, int64_t total, int world, int rank,
            const std::vector<std::pair<int64_t, int64_t>>& ps_ranges,
            const std::vector<int>& ps_host, int max_slices);
  ~AsyncPeer();
  std::string handle() const { return map_.handle(); }
  void open(const std::vector<std::string>& handles);
  void close();  // unmap peers, free buffers and the shm board (after a device drain); idempotent
  void unmap_peers() { map_.unmap_peers(); }  // the first half of close() alone (PeerMap)
  // worker: every PS shard of the gradient (x coef) into its host's inbox slot, round `epoch`
  void push_all(uint32_t epoch, float coef, hipStream_t st);
  // the same for the listed PS only (one launch); with_gate: plus the pull gate of round
  // `epoch` as the launch's last block (the round's last push, async_runner.hip)
  void push_set(const std::vector<int>& ps, uint32_t epoch, float coef, hipStream_t st,
                bool with_gate = false);
  // the same push as tail blocks of another launch (tail.h kind 1, one block per arrival
  // slice); false when the set does not fit a tail (more than kTailPieces shards)
  bool push_tail(const std::vector<int>& ps, uint32_t epoch, UpdTail& out) const;
  // the DONE counters and the arrival board: a POSIX shm segment (created by one rank,
  // attached by the others) registered with HIP, so every GPU stores into them and every host
  // polls them directly
  void attach_done(const std::string& name, bool create);
  // PS host: has `worker` posted round `epoch` of PS `ps`?  next_slice: the caller's scan
  // position (the first slice not yet seen posted; 0 for a new round)
  bool posted(int ps, int worker, uint32_t epoch, int& next_slice) const;
  // worker host: wait until every PS has stored round `epoch`'s parameters here (false on
  // timeout or a recorded kernel error)
  bool wait_done(uint32_t epoch, double timeout_s);
  // the same wait as one wave on stream `st` (the GPU-side pull gate, async_runner.hip)
  void gate(uint32_t epoch, hipStream_t st);
  // PS host: apply worker `worker`'s round-`epoch` push to PS `ps` (private copy ps_params,
  // optimizer state in u) and store the new shard into that worker's parameter buffer
  void apply(int ps, int worker, uint32_t epoch, const XgmiUpdate& u, float* ps_params,
             hipStream_t st);
  int error() const { return map_.error(); }
  int num_ps() const { return nps_; }
  // PS p's range of the parameter / gradient buffers and its host
  void shard(int p, int64_t& lo, int64_t& n, int& host) const;
  float* params() const { return params_; }
  const float* grads() const { return grads_; }

 private:
  void upload_table();           // table_ -> table_dev_ (set-up only: open, attach_done)
  float* params_;
  const float* grads_;
  int world_, rank_, nps_ = 0;
  AsyncTable table_;
  AsyncTable* table_dev_ = nullptr;  // the kernels' copy
  PeerMap map_;
  uint32_t* done_host_ = nullptr;
  uint32_t* posted_host_ = nullptr;
  size_t done_bytes_ = 0;
  std::string done_name_;
  bool done_owner_ = false;
};

class AsyncService {
 public:
  AsyncService(AsyncPeer* peer, int world, int device, const std::vector<AsyncPsState>& ps,
               const OptimSpec& opt, uint32_t epoch0, bool provenance);
  ~AsyncService();
  void start(int64_t expected);  // serve `expected` pushes on a native thread
  void join();                   // rethrows the thread's error, if any
  // checkpoint hook: no apply is issued between pause() and resume(), and every issued one has
  // completed when pause() returns (the PS state is one consistent step); same caller thread
  void pause();
  void resume();
  int64_t t(int ps) const { return bank_.t(ps); }
  int64_t served() const;
  // (worker, ps, worker round, PS step) per apply, in service order
  const std::vector<std::array<int64_t, 4>>& provenance() const { return bank_.provenance(); }
  // the thread scans the board and launches each apply
  const char* mode() const { return "host"; }

 private:
  void run();
  void serve(AsyncPsState& st, int worker);
  AsyncPeer* peer_;
  int world_, device_;
  PsBank bank_;                  // the hosted PS, their optimizer and the provenance log
  std::vector<uint32_t> epoch_;
  std::atomic<int64_t> served_{0};
  int64_t expected_ = 0;
  hipStream_t stream_ = nullptr;
  std::thread th_;
  std::string error_;
  mutable std::mutex pause_mu_;  // held by the service thread while it issues an apply
};

// Native asynchronous worker step over the xGMI data plane (async_runner.hip): wait for the
// previous round's parameters (host), forward, backward with each PS's gradient push launched
// after the segment that completes its range (the push posts itself on the arrival board).
class AsyncRunner {
 public:
  static constexpr int kSegments = 4;
  // seg_of_ps[p]: backward segment after which PS p's range is complete; epoch0: the round
  // already completed (the set-up self-test)
  AsyncRunner(Engine* eng, AsyncPeer* peer, int world, int rank, int device,
              const std::vector<int>& seg_of_ps, uint32_t epoch0);
  void step(const float* x, const int64_t* labels, int B, uint32_t seed, hipStream_t st,
            double timeout_s);
  // the last round's parameters are back
  void finish(double timeout_s);
  uint32_t epoch() const { return epoch_; }
  // pushes as tail blocks of the next segment's launch (default) or push kernels of their own
  void set_use_tail(bool on) { use_tail_ = on; }
  // the pull as a GPU-side gate before the next forward (default) or a host wait
  void set_gate(bool on) { gate_ = on; }
  // clip this worker's gradient by its global norm (clip.hip) before any push or in-line apply:
  // the whole backward runs first, with no tails, then the clip, then the pushes / applies in
  // segment order.  max_norm 0: off
  void set_clip(const ClipSite& c) { stage_.clip = c; }
  // accumulate the gradient over K micro-batches (accum.hip): K - 1 accumulate() calls, then
  // step(), whose backward runs whole, with no tails, ahead of the finish pass (the mean into the
  // gradient buffer), the clip if on, then the pushes / applies in segment order.  k 1: off
  void set_accum(const AccumSite& a) { stage_.accum = a; }
  // a non-final micro-batch: the start-of-step wait for the previous round's parameters (board
  // path), forward, the whole backward, the accumulate pass; no round, push, gate or apply
  void accumulate(const float* x, const int64_t* labels, int B, uint32_t seed, hipStream_t st,
                  double timeout_s);
  // In-line applies (one worker, every PS hosted by it, Adam): each push is applied on the
  // compute stream as Adam tail blocks of the next segment's launch — the last segment's inside
  // conv1's weight-gradient launch — with the PS's m / v and its own step counter t, in push
  // order.  A sole pusher's push order IS the arrival order, so no board claim, apply kernel,
  // DONE word or gate is needed; the PS's private parameter copy is not touched per step (it
  // equals the worker's buffer: inline_sync_ps() writes it back for checkpoints).  `ps` gives
  // every PS's m, v and t (its params pointer: the private copy).
  void set_inline(const std::vector<AsyncPsState>& ps, const OptimSpec& opt, bool provenance);
  bool inline_on() const { return inline_; }
  int64_t inline_t(int ps) const { return bank_.t(ps); }
  void inline_sync_ps(hipStream_t st);  // worker buffer -> every PS's private copy
  // (worker, ps, round, t) per in-line apply, when provenance was asked for
  const std::vector<std::array<int64_t, 4>>& inline_provenance() const {
    return bank_.provenance();
  }
  // stand-alone optimizer launches of the most recent in-line step (SyncRunner::update_launches)
  int update_launches() const { return upd_launches_ + eng_->update_launches; }

 private:
  void wait_round(double timeout_s);
  void check_round(uint32_t e, double timeout_s);
  void wait_params(double timeout_s);
  void step_inline(const MicroBatch& mb);
  float* grads() const { return const_cast<float*>(peer_->grads()); }
  bool inline_ = false;
  PsBank bank_;                    // in-line: every PS, under Adam or AdamW (no other rule)
  UpdatePlan plan_;                // in-line: one piece per PS, its shard with its own m / v
  int upd_launches_ = 0;
  std::vector<float> lr_t_;        // this round's TF1 Adam step size per PS
  hipStream_t last_st_ = nullptr;
  bool stepped_ = false;
  bool use_tail_ = true;
  bool gate_ = true;
  GradStage stage_;
  uint32_t gated_ = 0;  // the round the last step's gate waits for (0: none)
  WaitPlacement gate_place_;  // the pull gate on the compute stream against the service stream
  Engine* eng_;
  AsyncPeer* peer_;
  int world_, rank_, device_;
  uint32_t epoch_, epoch0_;
  std::vector<int> seg_ps_[kSegments];
};

// Asynchronous PS over point-to-point RCCL in exclusive sessions (rccl_async.hip): one
// communicator, one comm stream and one comm thread per process; a (worker, PS) round trip
// runs only while its initiator holds both processes' session locks.
class RcclAsync {
 public:
  RcclAsync(float* params, float* grads, int world, int rank, int device,
            const std::vector<std::pair<int64_t, int64_t>>& ps_ranges,
            const std::vector<int>& hosts, const std::vector<AsyncPsState>& hosted,
            const OptimSpec& opt, bool self_sessions);
  ~RcclAsync();
  void init_comm(const char id[128]);               // collective over all ranks
  void attach_shm(const std::string& job, bool create);  // session locks (rank 0 creates)
  void open_boxes(bool own);                        // own: create mine; else attach the others
  void start(int64_t expected_served, bool provenance);
  void push_pull(hipStream_t compute);              // this worker's round (blocks the caller)
  void join();
  void pause();
  void resume();
  int64_t t(int ps) const { return bank_.t(ps); }
  // a hosted PS's step counter before start() (resume: the checkpoint's t, restored after the
  // object was built — Adam's bias correction continues instead of restarting at t = 1)
  void set_t(int ps, int64_t t);
  int64_t served() const { return served_.load(); }
  // (worker, ps, that worker's round at this PS, PS step) per applied push
  const std::vector<std::array<int64_t, 4>>& provenance() const { return bank_.provenance(); }

 private:
  void loop();
  bool push_one(int p);
  void serve(int worker, int p);
  void apply(int p, int worker, const float* g);
  float* w_;
  float* g_;
  int world_, rank_, device_;
  std::vector<std::pair<int64_t, int64_t>> ranges_;
  std::vector<int> hosts_;
  PsBank bank_;                  // (rule scale 1: the workers push unscaled gradients)
  bool self_;
  void* comm_ = nullptr;
  hipStream_t cs_ = nullptr;
  hipEvent_t ev_ = nullptr;
  float* gbuf_ = nullptr;
  SessionLocks locks_;  // runtime/session.h (CPU-stress-tested protocol)
  std::string box_name_;
  std::unique_ptr<ShmMailbox> mine_;
  std::unique_ptr<ShmMailbox> boxes_[kXgmiMaxPeers];
  std::vector<int64_t> count_;
  std::atomic<int64_t> served_{0};
  int64_t expected_ = 0;
  std::thread th_;
  std::mutex qmu_;               // round queue / stop / error
  std::mutex pause_mu_;
  std::condition_variable cv_;
  std::vector<int> pending_;
  bool waited_ = false;
  bool stop_ = false;
  std::string error_;
};

class SyncRunner {
 public:
  static constexpr int kSegments = 4;
  SyncRunner(Engine* eng, float* params, float* grads, int world, int rank);
  ~SyncRunner();
  static void unique_id(char out[128]);
  // "" when torch's librccl and every entry point the runner uses resolve, else the reason
  static std::string probe();
  // collective over all ranks; W = 1 only with `force` (1-rank communicator: the collective
  // units then run as RCCL copies — the on-device test of the exchange path on one GPU)
  void init_comm(const char id[128], bool force = false);
  bool has_comm() const { return comm_ != nullptr; }
  void set_units(const std::vector<RunnerUnit>& units);
  // Adam or momentum; the rule's scale stays set_scale's.  A modified rule rides wherever its
  // base rule does: the tail-path conditions test the kind only.
  void set_optimizer(const OptimSpec& opt);
  void set_scale(float grad_scale, float coef) { opt_.rule.scale = grad_scale; coef_ = coef; }
  // clip this worker's gradient by its global norm (clip.hip) after the fourth backward segment
  // and before anything consumes it.  The caller maps every unit to the last segment; the tail
  // and final-in-reduce placements are not taken, as with coef_ != 1.  max_norm 0: off
  void set_clip(const ClipSite& c) { stage_.clip = c; }
  // accumulate the gradient over K micro-batches (accum.hip): K - 1 accumulate() calls, then
  // step(), which runs as a clipped step does (every unit on the last segment) with the finish
  // pass — the mean into the gradient buffer — ahead of the clip.  k 1: off
  void set_accum(const AccumSite& a) { stage_.accum = a; }
  // a non-final micro-batch: forward, the whole backward, the accumulate pass, nothing else
  void accumulate(const float* x, const int64_t* labels, int B, uint32_t seed, hipStream_t st);
  // one synchronous training step on stream `st`; lr_t indexed by RunnerUnit::ps
  void step(const float* x, const int64_t* labels, int B, uint32_t seed, const float* lr_t,
            hipStream_t st);
  bool selftest(std::string* why);
  void set_local_on_main(bool on) { local_on_main_ = on; }
  // collective units of the LAST backward segment on the compute stream (no event hop on the
  // step's critical path; RCCL still orders them after the comm stream's earlier units)
  void set_last_on_main(bool on) { last_on_main_ = on; }
  std::string async_error();  // "" while the communicator is healthy (RCCL and xGMI)
  // XGMI units exchange through this (owned by the caller; outlives the runner's use)
  PeerExchange* peer() const { return peer_; }
  void set_peer(PeerExchange* p) {
    peer_ = p;
    if (p) p->set_gate_error(ready_err_dev());  // (device memory: read by every bucket wave)
  }
  int* ready_err_dev() const { return ready_ ? reinterpret_cast<int*>(ready_ + kSegments) : nullptr; }
  // one full exchange of every bucket with w := sum over ranks of g (no optimizer) at the
  // next epoch; the caller fills g, checks w
  void peer_selftest_step(hipStream_t st);
  void abort();               // ncclCommAbort: unblocks this rank's pending collectives
  // orderly ncclCommDestroy (call on every rank at the same point), then release()
  void close();
  hipStream_t comm_stream() const { return cs_; }
  // stand-alone optimizer kernel launches (update / gradient scale / a flushed update tail)
  // issued for the most recent step(): 0 when every update rode in a backward launch.  Counted
  // on the host; diagnostic only
  int update_launches() const { return upd_launches_ + eng_->update_launches; }

 private:
  void issue(const RunnerUnit& u, const float* lr_t, hipStream_t st);
  // all REDUCE units of one segment: one RCCL group of reduces, the hosted updates, one
  // group of broadcasts (instead of two groups per unit)
  void issue_reduce_group(const std::vector<const RunnerUnit*>& us, const float* lr_t,
                          hipStream_t st);
  void update(const UpdSpan& s, const float* g, int64_t n, float lr_t, hipStream_t st);
  void scale_grads(float* p, int64_t n, hipStream_t st);  // g *= coef_
  int upd_launches_ = 0;
  void issue_xgmi(const RunnerUnit& u, const float* lr_t, bool final_wait, hipStream_t st,
                  bool gated = false);
  int last_xgmi_ = -1;     // index of the step's last XGMI unit (carries the final wait)
  void release();          // destroy the comm stream, events and flags (idempotent)
  bool closed_ = false;
  Engine* eng_;
  float* w_;
  float* g_;
  int world_, rank_;
  void* comm_ = nullptr;  // ncclComm_t
  PeerExchange* peer_ = nullptr;
  uint32_t epoch_ = 0;     // xGMI flag epoch: one per step, identical on every rank
  hipStream_t cs_ = nullptr;
  hipEvent_t seg_ev_[kSegments] = {};
  hipEvent_t seg_ev_dev_[kSegments] = {};  // device-scope release (xGMI-only segments)
  bool seg_xgmi_only_[kSegments] = {};
  // segments with exchange units on the comm stream (xGMI or RCCL) hand their gradients over
  // by a READY flag (tail.h kind 2) instead of an event: 0 never, 1 every segment but the
  // first, 2 every segment (default: forced xGMI rehearsal 0.3156 / 0.3164 / 0.3058 ms/step,
  // scripts/ready_ab.py)
  int ready_flags_ = 2;
  bool seg_offstream_[kSegments] = {};     // the segment has units on the comm stream
  int seg_launches_[kSegments] = {};       // kernel launches of the segment in the last step
  // seg events recorded by the segment's own kernel packets (DDL_EXT_EVENT, default on)
  bool ext_event_ = true;
  hipEvent_t done_ev_ = nullptr;
  // the READY gate on the comm stream (the greatest priority, or the least with
  // DDL_COMM_PRIORITY=low) waits for a kernel of the compute stream; else the event hand-off
  WaitPlacement gate_place_;
  uint32_t* ready_ = nullptr;     // READY[segment] (uncached device memory, tail.h kind 2)
  int* ready_err_ = nullptr;      // a READY gate timed out (host memory)
  double gate_timeout_s_ = 20.0;  // DDL_XGMI_TIMEOUT_S
  uint32_t ready_epoch_ = 0;      // one per step
  std::vector<RunnerUnit> units_;
  // (scale: set_scale's grad_scale; Adam's lr_t comes with every step())
  OptimSpec opt_ = OptimSpec::from_doubles(kUpdAdam, 1e-4f, 0.9, 0.999, 1e-8f, 0.9f, 1.f);
  float coef_ = 1.f;
  GradStage stage_;
  // a range's parameter / optimizer-state span (state at state_off of the owning PS's m / v)
  UpdSpan span_of(const RunnerRange& r, float* m, float* v) const {
    return UpdSpan{w_ + r.lo, m + r.state_off, v ? v + r.state_off : nullptr};
  }
  bool local_on_main_ = true;
  bool last_on_main_ = true;
  bool all_local_ = false;
  UpdatePlan plan_;  // all_local_: where the LOCAL updates go (update_plan.h)
  bool use_tail_ = true;
  bool final_in_reduce_ = env_flag("DDL_FINAL_IN_REDUCE", true);

 public:
  void set_ready_flags(int mode) { ready_flags_ = mode; }
  void set_use_tail(bool on) { use_tail_ = on; }
  // the last segment's update inside conv1's weight-gradient launch (tail path only): with the
  // direct conv1 kernel conv2's Adam runs in its weight-gradient reduce epilogue and conv1's in
  // the final reduce level (engine_impl.h final_split_conv12): 0.2988 -> 0.2973 ms/step; with
  // the GEMM conv1 path as tail blocks of the wide reduce (measured neutral).
  // DDL_FINAL_IN_REDUCE=0: the stand-alone Adam launch
  void set_final_in_reduce(bool on) { final_in_reduce_ = on; }
  // tail placement (1: before the GEMM blocks) and float4 per tail block (tuning)
  void set_tail_cfg(int first, int f4_per_block) {
    tail_first_ = first;
    tail_f4_ = std::max(1, f4_per_block / kTailF4PerBlock) * kTailF4PerBlock;
  }

 private:
  // measured (scripts/tail_probe.py, one MI355X): after the GEMM blocks, 512 float4 per
  // block: 373 us/step vs 381 without the tail; before the GEMM blocks 375-378
  int tail_first_ = 0;
  int tail_f4_ = kTailF4Default;
};

}  // namespace ddl
