// Native synchronous training-step runner: forward, the four backward segments, and the
// per-unit gradient exchange + PS update, all enqueued from C++ (one Python call per step).
//
// Reference behaviour (SURVEY.md §2.7 sync data plane; mnist_sync_sharding/worker.py:95-120,
// parameter_server.py:108-126): every worker pushes its gradients to the owning PS, the PS
// applies Adam once per global step and every worker pulls the new parameters.  Here:
//
//  * a unit = a set of plan-buffer ranges whose gradients are complete after backward segment
//    `seg`; the comm stream waits on that segment's event, so the exchange of the fc layers
//    runs while the conv backward is still computing (bucketed overlap);
//  * kind LOCAL  : this rank owns the PS of the ranges (W = 1, or co-located) -> fused Adam;
//  * kind RS     : flat plan with one PS per GPU: ncclReduceScatter -> fused Adam on this
//                  rank's 1/W chunk -> in-place ncclAllGather (ring-optimal on xGMI);
//  * kind REDUCE : tensor-granular plans: ncclReduce(dst=host) -> Adam at the host ->
//                  ncclBroadcast(src=host), ranges of a unit grouped in one RCCL group.
//
// The communicator is our own RCCL comm (torch's librccl instance, id exchanged through
// torch.distributed), so the per-step host cost is a few launches instead of one Python
// ProcessGroup call per collective — the Python exchange was host-bound (step timeline:
// 20-45 us GPU idle at every segment boundary).

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "api.h"
#include "common.h"
#include "rccl_api.h"
#include "trace.h"

namespace ddl {

static ncclComm_t as_comm(void* c) { return reinterpret_cast<ncclComm_t>(c); }

// One wave on the comm stream ahead of segment s's exchange units: returns once the compute
// stream has started segment s+1 (READY[s] >= epoch, stored by that launch's first tail block,
// tail.h kind 2), i.e. once every launch of segment s has completed — a kernel boundary writes
// the producer's dirty L2 lines back, so the gradients are in memory for this GPU's exchange
// kernels and for a peer's P2P reads alike.  The comm stream has a priority of its own, so this wait
// never shares a hardware queue with the kernel that releases it.  Bounded (error word).
// On a timeout it also raises the device copy of the error (err_dev, uncached device memory),
// which the gated xGMI bucket kernels behind it read — a host-memory word read by every wave of
// a 512-block bucket kernel was ~2,000 PCIe reads per launch: the forced xGMI rehearsal ran
// 0.49 instead of 0.30 ms/step, the GEMMs beside it ~7x slower.
__global__ void __launch_bounds__(64) ready_gate_kernel(const uint32_t* flag, uint32_t epoch,
                                                        int* err, int* err_dev,
                                                        long long timeout_ticks) {
  if (threadIdx.x != 0) return;
  const long long deadline = wall_clock64() + timeout_ticks;
  // a long sleep between polls (~0.5 us): the first segment's gate of the next step is issued
  // while that step's forward runs, and a tight poll slowed the forward GEMMs by ~20 %
  for (int it = 0;
       (int32_t)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0;
       ++it) {
    if ((it & 15) == 15 && wall_clock64() > deadline) {
      __hip_atomic_store(err_dev, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    __builtin_amdgcn_s_sleep(16);
  }
}

// ---- shared with the asynchronous runner (async_runner.hip) -------------------------------------
void run_forward(Engine& eng, const MicroBatch& mb) {
  TraceRange r("ddl.fwd");
  // (dropout seed by kernel argument, Engine::seed_value: no seed-upload kernel, no seed word)
  eng.forward(mb.x, mb.B, nullptr, true, mb.st, /*defer_fc2=*/true);  // backward_segment(0) follows
}

void run_whole_backward(Engine& eng, const MicroBatch& mb) {
  for (int s = 0; s < kPlanSegments; ++s) {
    TraceRange r(mb.bwd_range[s]);
    eng.backward_segment(s, mb.x, mb.labels, mb.B, nullptr, mb.st);
  }
  eng.flush_tail(mb.st);  // (no-op with nothing pending)
}

int launch_piece_updates(const LocalUpdates& u, const std::vector<PlanPiece>& pieces,
                         hipStream_t st) {
  int launches = 0;
  for (const auto& p : pieces) {
    const UpdSpan span{u.w + p.lo, p.m + p.state_off, p.v ? p.v + p.state_off : nullptr};
    launch_update(u.opt->rule, u.step(p), span, u.g + p.lo, p.n(), st, u.max_grid);
    launches += p.n() > 0;
  }
  return launches;
}

// `pieces` under u's rule as one optimizer tail (at most kTailPieces of them).  Momentum: v stays
// null and is never formed.
static UpdTail tail_of(const LocalUpdates& u, const std::vector<PlanPiece>& pieces, int first,
                       int f4_per_block) {
  UpdTail t;
  t.rule = u.opt->rule;
  t.first = first;
  t.f4_per_block = f4_per_block;
  for (const auto& p : pieces) {
    UpdPiece q;
    q.w = u.w + p.lo;
    q.g = u.g + p.lo;
    q.m = p.m + p.state_off;
    q.v = u.opt->rule.kind == kUpdMomentum ? nullptr : p.v + p.state_off;
    q.n = p.n();
    q.step = u.step(p);
    t.add_piece(q);
  }
  t.finish();
  return t;
}

int run_riding_backward(Engine& eng, const MicroBatch& mb, const LocalUpdates& u,
                        const RidePolicy& pol) {
  const auto* seg = u.plan->seg;
  const int last = kPlanSegments - 1;
  int launches = 0;
  for (int s = 0; s < kPlanSegments; ++s) {
    TraceRange r(mb.bwd_range[s]);
    if (s > 0 && !seg[s - 1].empty()) {
      if (pol.rides[s - 1]) eng.tail = tail_of(u, seg[s - 1], pol.first, pol.f4_per_block);
      else launches += launch_piece_updates(u, seg[s - 1], mb.st);
    }
    // one pass per tail block (2 float4 per lane): on the step's critical path the update wants
    // width, not the long blocks that hide beside a dual launch's GEMM blocks
    if (s == last && pol.final_in_reduce && pol.rides[s] && !seg[s].empty())
      eng.final_upd = tail_of(u, seg[s], pol.first, kTailF4PerBlock);
    eng.backward_segment(s, mb.x, mb.labels, mb.B, nullptr, mb.st);
    eng.flush_tail(mb.st);
  }
  const bool offered = pol.final_in_reduce && pol.rides[last];
  if (seg[last].empty() || (offered && eng.final_upd.npieces == 0)) return launches;  // taken
  eng.final_upd = UpdTail();  // not taken by conv1's launch: launches of its own
  TraceRange r("ddl.update.last_segment");
  return launches + launch_piece_updates(u, seg[last], mb.st);
}

SyncRunner::SyncRunner(Engine* eng, float* params, float* grads, int world, int rank)
    : eng_(eng), w_(params), g_(grads), world_(world), rank_(rank) {
  int lo = 0, hi = 0;
  HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  // collectives + optimizer on a high-priority stream so they are not starved by the GEMMs
  // (DDL_COMM_PRIORITY=low: the least priority instead — also a pool of its own, so the READY
  // gate's argument holds; A/B for ranks sharing a card)
  const char* cp = getenv("DDL_COMM_PRIORITY");
  HIP_CHECK(hipStreamCreateWithPriority(&cs_, hipStreamNonBlocking,
                                        cp && cp[0] == 'l' ? lo : hi));
  // The segment events hand gradients written by this device's GEMMs to RCCL kernels on this
  // device.  On the 1-rank rehearsal (W = 1, every collective a local copy) a device-scope
  // release suffices and removed a ~7 us gap per backward segment (forced 1-rank timeline).
  // With W > 1, RCCL's P2P transports may read these buffers from a peer GPU, and the relaxed
  // fence has not been validated there, so W > 1 keeps the system-scope fence.  The
  // end-of-exchange event keeps the system scope: it orders the next forward after collectives
  // that received peer data, and it is recorded on the comm stream, off the compute stream's
  // critical path.
  const bool sysfence = world_ > 1;
  const unsigned ev_flags =
      hipEventDisableTiming | (sysfence ? 0u : (unsigned)hipEventDisableSystemFence);
  for (int s = 0; s < kSegments; ++s) {
    HIP_CHECK(hipEventCreateWithFlags(&seg_ev_[s], ev_flags));
    // xGMI units: the consumer of the segment's gradients is our own kernel on this device
    // (peers never read them: the exchange pushes), so a device-scope release is exact at
    // any world size
    HIP_CHECK(hipEventCreateWithFlags(&seg_ev_dev_[s],
                                      hipEventDisableTiming | hipEventDisableSystemFence));
  }
  HIP_CHECK(hipEventCreateWithFlags(&done_ev_, hipEventDisableTiming));
  // READY[s] words, then the device copy of the gate's error word
  HIP_CHECK(hipExtMallocWithFlags(reinterpret_cast<void**>(&ready_),
                                  (kSegments + 1) * sizeof(uint32_t), hipDeviceMallocUncached));
  HIP_CHECK(hipMemset(ready_, 0, (kSegments + 1) * sizeof(uint32_t)));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ready_err_), 64, hipHostMallocDefault));
  memset(ready_err_, 0, 64);
  HIP_CHECK(hipDeviceSynchronize());
  ext_event_ = env_flag("DDL_EXT_EVENT", true, /*only_1=*/true);
  // the READY gate is bounded like the xGMI waits (the same setting and default)
  gate_timeout_s_ = xgmi_timeout_s(20.0);
}

SyncRunner::~SyncRunner() {
  if (comm_) {
    (void)rccl().CommDestroy(as_comm(comm_));
    --rccl_live_comms();
  }
  comm_ = nullptr;
  release();
}

// Every HIP object the runner owns: the comm stream (a hardware queue of its own priority), the
// events, the READY flags.  Idempotent; after it the runner refuses to step.
void SyncRunner::release() {
  if (cs_) (void)hipStreamSynchronize(cs_);
  if (peer_) peer_->set_gate_error(nullptr);
  for (int s = 0; s < kSegments; ++s) {
    if (seg_ev_[s]) (void)hipEventDestroy(seg_ev_[s]);
    if (seg_ev_dev_[s]) (void)hipEventDestroy(seg_ev_dev_[s]);
    seg_ev_[s] = seg_ev_dev_[s] = nullptr;
  }
  if (done_ev_) (void)hipEventDestroy(done_ev_);
  done_ev_ = nullptr;
  if (ready_) (void)hipFree(ready_);
  ready_ = nullptr;
  if (ready_err_) (void)hipHostFree(ready_err_);
  ready_err_ = nullptr;
  if (cs_) (void)hipStreamDestroy(cs_);
  cs_ = nullptr;
  closed_ = true;
}

void SyncRunner::unique_id(char out[128]) {
  ncclUniqueId id;
  RCCL_CHECK(rccl().GetUniqueId(&id));
  static_assert(sizeof(id) == 128, "ncclUniqueId size");
  memcpy(out, &id, 128);
}

std::string SyncRunner::probe() {
  // (an override table is a test's stand-in, never a library a job may train on)
  if (rccl_overridden()) return "an RCCL override table is installed";
  try {
    (void)rccl();
  } catch (const std::exception& e) {
    return e.what();
  }
  return std::string();
}

void SyncRunner::init_comm(const char id_bytes[128], bool force) {
  if (world_ <= 1 && !force) return;
  ncclUniqueId id;
  memcpy(&id, id_bytes, 128);
  ncclComm_t c;
  RCCL_CHECK(rccl().CommInitRank(&c, world_, id, rank_));
  comm_ = c;
  ++rccl_live_comms();
}

void SyncRunner::set_units(const std::vector<RunnerUnit>& units) {
  for (const auto& u : units) {
    if (u.seg < 0 || u.seg >= kSegments) throw std::invalid_argument("unit segment out of range");
    const bool xg = u.kind == RunnerUnit::XGMI || u.kind == RunnerUnit::XGMI_REPL;
    if (u.kind != RunnerUnit::LOCAL && !xg && !comm_)
      throw std::invalid_argument("collective unit without an RCCL communicator");
    if (u.kind == RunnerUnit::AR && u.ranges.size() != 1)
      throw std::invalid_argument("all-reduce unit needs exactly one range");
    if (u.kind == RunnerUnit::RS && (u.ranges.size() != 1 || !u.shard))
      throw std::invalid_argument("RS unit needs exactly one range and a shard buffer");
    if (u.kind == RunnerUnit::RS && (u.ranges[0].hi - u.ranges[0].lo) % world_ != 0)
      throw std::invalid_argument("RS unit range not divisible by the world size");
    if (xg) {
      if (!peer_) throw std::invalid_argument("xGMI unit without a PeerExchange");
      if (u.bucket < 0 || u.bucket >= peer_->num_buckets())
        throw std::invalid_argument("xGMI unit bucket out of range");
      if ((u.kind == RunnerUnit::XGMI_REPL) != (u.bucket == peer_->repl_bucket()))
        throw std::invalid_argument("xGMI unit kind does not match the exchange's replicated bucket");
      // the replicated kernel has no DONE words (the final wait cannot see it) and reuses its
      // parity slots on the next-but-one step: only the compute stream's program order after
      // the last backward segment makes both safe
      if (u.kind == RunnerUnit::XGMI_REPL && u.seg != kSegments - 1)
        throw std::invalid_argument("the replicated xGMI bucket must be the last segment's");
      // (an owner bucket's optimizer state exists only on its owner rank)
      const bool owns = peer_->owner(u.bucket) < 0 || peer_->owner(u.bucket) == rank_;
      if (owns && opt_.rule.kind == kUpdAdam && !u.v) throw std::invalid_argument("xGMI unit without Adam state");
      if (peer_->owner(u.bucket) >= 0 && peer_->owner(u.bucket) != u.host)
        throw std::invalid_argument("xGMI owner bucket hosted on another rank than its unit");
    }
  }
  units_ = units;
  // segments whose off-stream units are all xGMI take the device-scope event
  for (int sg = 0; sg < kSegments; ++sg) {
    bool any = false, only = true;
    for (const auto& u : units_)
      if (u.seg == sg && !(u.kind == RunnerUnit::LOCAL && local_on_main_)) {
        any = true;
        only &= u.kind == RunnerUnit::XGMI || u.kind == RunnerUnit::XGMI_REPL;
      }
    seg_xgmi_only_[sg] = any && only;
    seg_offstream_[sg] = any;
  }
  // the step's last xGMI unit also waits until every owner's parameters have landed here
  last_xgmi_ = -1;
  for (size_t i = 0; i < units_.size(); ++i)
    if ((units_[i].kind == RunnerUnit::XGMI || units_[i].kind == RunnerUnit::XGMI_REPL) &&
        (last_xgmi_ < 0 || units_[i].seg >= units_[last_xgmi_].seg))
      last_xgmi_ = (int)i;
  // W = 1 (every unit LOCAL): one stream, the updates planned by update_plan.h
  plan_ = UpdatePlan();
  all_local_ = true;
  for (const auto& u : units_) all_local_ &= (u.kind == RunnerUnit::LOCAL);
  if (!all_local_) return;
  for (const auto& u : units_)
    for (const auto& r : u.ranges)
      plan_.add(u.seg, PlanPiece{r.lo, r.hi, r.state_off, u.ps, u.m, u.v});
  plan_.finish(reinterpret_cast<uintptr_t>(w_), reinterpret_cast<uintptr_t>(g_));
}

void SyncRunner::set_optimizer(const OptimSpec& opt) {
  if (opt.rule.kind != kUpdAdam && opt.rule.kind != kUpdMomentum)
    throw std::invalid_argument("native runner: adam or momentum");
  const float scale = opt_.rule.scale;
  opt_ = opt;
  opt_.rule.scale = scale;
}

// An update on the comm stream overlaps the backward's dual launches: fewer workgroups leave
// the slots those free to the duals (as the xGMI bucket kernels' cap, native_exchange.py).
// Forced RCCL rehearsal, 300-step bench: 2048 / 512 / 256 / 128 / 64 workgroups: 0.2762-0.2771 /
// 0.2745-0.2755 / 0.2723-0.2741 / 0.2717-0.2718 / 0.2752-0.2756 ms/step
// (profiles/r6_comm_adam_grid.log)
#ifndef DDL_COMM_ADAM_GRID
#define DDL_COMM_ADAM_GRID 128
#endif
void SyncRunner::update(const UpdSpan& s, const float* g, int64_t n, float lr_t, hipStream_t st) {
  const int max_grid = st == cs_ ? DDL_COMM_ADAM_GRID : 2048;
  launch_update(opt_.rule, opt_.step_for(lr_t), s, g, n, st, max_grid);
  upd_launches_ += n > 0;
}

// launch_scale of the coefficient path, counted like update()
void SyncRunner::scale_grads(float* p, int64_t n, hipStream_t st) {
  launch_scale(p, n, coef_, st);
  upd_launches_ += n > 0;
}

void SyncRunner::issue(const RunnerUnit& u, const float* lr_t, hipStream_t st) {
  if (u.kind == RunnerUnit::REDUCE) {
    issue_reduce_group({&u}, lr_t, st);
    return;
  }
  if (coef_ != 1.f)
    for (const auto& r : u.ranges) scale_grads(g_ + r.lo, r.hi - r.lo, st);
  const float lt = lr_t[u.ps];
  switch (u.kind) {
    case RunnerUnit::LOCAL:
      for (const auto& r : u.ranges)
        update(span_of(r, u.m, u.v), g_ + r.lo, r.hi - r.lo, lt, st);
      break;
    case RunnerUnit::RS: {
      const auto& r = u.ranges[0];
      const int64_t c = (r.hi - r.lo) / world_;
      float* mine = w_ + r.lo + rank_ * c;
      RCCL_CHECK(rccl().ReduceScatter(g_ + r.lo, u.shard, (size_t)c, ncclFloat32, ncclSum,
                                   as_comm(comm_), st));
      UpdSpan s = span_of(r, u.m, u.v);
      s.w = mine;
      update(s, u.shard, c, lt, st);
      RCCL_CHECK(rccl().AllGather(mine, w_ + r.lo, (size_t)c, ncclFloat32, as_comm(comm_), st));
    } break;
    case RunnerUnit::AR: {
      // the step's last bucket, replicated: ONE all-reduce, then every rank runs the update on
      // its replicated optimizer state (one collective instead of reduce-scatter + all-gather
      // on the exposed end of the step)
      const auto& r = u.ranges[0];
      const int64_t n = r.hi - r.lo;
      RCCL_CHECK(rccl().AllReduce(g_ + r.lo, g_ + r.lo, (size_t)n, ncclFloat32, ncclSum,
                                  as_comm(comm_), st));
      update(span_of(r, u.m, u.v), g_ + r.lo, n, lt, st);
    } break;
    default:
      throw std::invalid_argument("unknown unit kind");
  }
}

// Tensor-granular plans put the units of one backward segment on different hosts (e.g. at
// W = 8 contiguous: conv4 weight on PS 6, its bias on PS 7).  Grouping every reduce of the
// segment lets RCCL run them as one launch with the roots' transfers concurrent on
// different xGMI links, then every broadcast likewise: 2 collective launches per segment
// instead of 2 per unit (each launch costs ~10-20 us of latency on an 8-GPU ring).
void SyncRunner::issue_reduce_group(const std::vector<const RunnerUnit*>& us, const float* lr_t,
                                    hipStream_t st) {
  for (const RunnerUnit* u : us)
    if (coef_ != 1.f)
      for (const auto& r : u->ranges) scale_grads(g_ + r.lo, r.hi - r.lo, st);
  RCCL_CHECK(rccl().GroupStart());
  for (const RunnerUnit* u : us)
    for (const auto& r : u->ranges)
      RCCL_CHECK(rccl().Reduce(g_ + r.lo, g_ + r.lo, (size_t)(r.hi - r.lo), ncclFloat32, ncclSum,
                               u->host, as_comm(comm_), st));
  RCCL_CHECK(rccl().GroupEnd());
  for (const RunnerUnit* u : us)
    if (rank_ == u->host)
      for (const auto& r : u->ranges)
        update(span_of(r, u->m, u->v), g_ + r.lo, r.hi - r.lo, lr_t[u->ps], st);
  RCCL_CHECK(rccl().GroupStart());
  for (const RunnerUnit* u : us)
    for (const auto& r : u->ranges)
      RCCL_CHECK(rccl().Broadcast(w_ + r.lo, w_ + r.lo, (size_t)(r.hi - r.lo), ncclFloat32,
                                  u->host, as_comm(comm_), st));
  RCCL_CHECK(rccl().GroupEnd());
}

static const char* const kBwdRange[SyncRunner::kSegments] = {
    "ddl.bwd.seg0(head+fc)", "ddl.bwd.seg1(conv4)", "ddl.bwd.seg2(conv3)",
    "ddl.bwd.seg3(conv2+conv1)"};
static const char* const kExRange[SyncRunner::kSegments] = {
    "ddl.exchange.seg0", "ddl.exchange.seg1", "ddl.exchange.seg2", "ddl.exchange.seg3"};

void SyncRunner::step(const float* x, const int64_t* labels, int B, uint32_t seed_value,
                      const float* lr_t, hipStream_t st) {
  if (closed_) throw std::runtime_error("sync runner: step() after close()");
  TraceRange step_range("ddl.step");
  upd_launches_ = eng_->update_launches = 0;  // (host counters: update_launches())
  stage_.accum.expect(true);
  const bool whole = stage_.whole();
  if (whole)
    for (const auto& u : units_)
      if (u.seg != kSegments - 1)
        throw std::invalid_argument("sync runner: a clipped step needs every unit on the last segment");
  eng_->seed_value = seed_value;  // dropout seed by kernel argument: no seed-upload kernel
  const uint32_t* seed = nullptr;
  const MicroBatch mb{x, labels, B, st, kBwdRange};
  // Cross-queue dependencies (event record -> stream wait) cost tens of microseconds of GPU
  // idle each on this stack (measured), so LOCAL updates go straight onto the compute
  // stream in order; only units with collectives use the comm stream, which then overlaps
  // the remaining backward segments.
  run_forward(*eng_, mb);
  if (all_local_ && local_on_main_) {
    const LocalUpdates u{&plan_, &opt_, lr_t, w_, g_, st == cs_ ? DDL_COMM_ADAM_GRID : 2048};
    // (Adam needs every piece's v; momentum / SGD have none and form none)
    if (use_tail_ && plan_.tail_ok && (opt_.rule.kind == kUpdMomentum || plan_.tail_v_ok) &&
        coef_ == 1.f && !whole) {
      const RidePolicy all_ride{{true, true, true, true}, tail_first_, tail_f4_, final_in_reduce_};
      upd_launches_ += run_riding_backward(*eng_, mb, u, all_ride);
      return;
    }
    run_whole_backward(*eng_, mb);
    stage_.finish(g_, st);  // the mean over the K micro-batches, then the clip
    TraceRange r("ddl.update");
    if (coef_ != 1.f)
      for (const auto& p : plan_.merged) scale_grads(g_ + p.lo, p.n(), st);
    upd_launches_ += launch_piece_updates(u, plan_.merged, st);
    return;
  }
  // The last segment's gradients complete with the backward, so nothing is left to overlap
  // its exchange with: its collectives go in order on the compute stream (no event record /
  // stream wait between the final backward launch, the exchange and the next forward).
  bool comm_used = false;
  if (__atomic_load_n(ready_err_, __ATOMIC_ACQUIRE))
    throw std::runtime_error("sync runner: a READY gate timed out (a segment never completed)");
  ++ready_epoch_;
  if (last_xgmi_ >= 0) {
    if (const int e = peer_->error())
      throw std::runtime_error("xGMI exchange timed out waiting for a peer (code " +
                               std::to_string(e) + ")");
    ++epoch_;
  }
  std::vector<const RunnerUnit*> reduces;
  for (int s = 0; s < kSegments; ++s) {
    const bool on_main = last_on_main_ && s == kSegments - 1;
    hipEvent_t ev = seg_xgmi_only_[s] ? seg_ev_dev_[s] : seg_ev_[s];
    // xGMI-only segment followed by another: the hand-off to the comm stream is a READY flag
    // stored by the next segment's first launch (tail.h kind 2) and a one-wave gate ahead of the
    // bucket kernels on the comm stream — no event record / stream wait (each left ~5 us of
    // idle compute stream: profiles/r4_step_timeline_forced_xgmi.txt).  The comm stream has
    // high priority, so the gate never shares a hardware queue with the kernel it waits for;
    // and it is bounded (error 5).
    const bool flag = ready_flags_ > (s == 0 ? 1 : 0) && !on_main && seg_offstream_[s] &&
                      s + 1 < kSegments && gate_place_.safe(st, cs_);
    // otherwise the comm stream waits for this segment's gradients by an event: bound to the
    // segment's kernel launches themselves (the wait below is issued after the last one) rather
    // than a marker packet behind them
    // (a clipped step's gradients are complete only after the clip, which follows the segment's
    // launches: a marker record behind it, not an event bound to the segment's last launch)
    const bool bind = ext_event_ && !on_main && seg_offstream_[s] && !flag && !whole;
    // bound to the segment's LAST launch (its count is learned from the previous step; a
    // wrong or unknown count falls back to a marker record below, which supersedes the binding)
    bool marker = !bind;
    {
      TraceRange r(kBwdRange[s]);
      StopEventScope scope(bind ? ev : nullptr, seg_launches_[s] > 0 ? seg_launches_[s] - 1
                                                                      : 1 << 30);
      eng_->backward_segment(s, x, labels, B, seed, st);
      if (bind) {
        const int n = scope.launches();
        if (scope.bound() != n - 1) marker = true;
        seg_launches_[s] = n;
      }
    }
    // every unit is the last segment's (checked above): the worker's own clipped gradient is
    // what every exchange and update below reads
    if (whole && s == kSegments - 1) {
      eng_->flush_tail(st);  // (nothing pending: no segment before the last handed anything over)
      stage_.finish(g_, st);
    }
    TraceRange ex_range(kExRange[s]);
    hipStream_t xs = on_main ? st : cs_;
    bool waited = on_main;
    reduces.clear();
    for (size_t i = 0; i < units_.size(); ++i) {
      const auto& u = units_[i];
      if (u.seg != s) continue;
      if (u.kind == RunnerUnit::LOCAL && local_on_main_) {
        issue(u, lr_t, st);
        continue;
      }
      if (!waited) {
        if (flag) {
          eng_->flush_tail(st);  // (no update tail is pending at W > 1; keep the slot free)
          UpdTail t;
          t.kind = 2;
          t.epoch = ready_epoch_;
          t.npieces = 1;
          t.p[0].arrive = ready_ + s;
          t.nblocks = 8;
          t.first = 1;
          eng_->tail = t;
          hipLaunchKernelGGL(ready_gate_kernel, dim3(1), dim3(64), 0, cs_, ready_ + s,
                             ready_epoch_, ready_err_, ready_err_dev(),
                             (long long)(gate_timeout_s_ * 1e8));
          DDL_CHECK_LAUNCH();
        } else {
          if (marker) HIP_CHECK(hipEventRecord(ev, st));
          HIP_CHECK(hipStreamWaitEvent(cs_, ev, 0));
        }
        waited = true;
      }
      if (u.kind == RunnerUnit::XGMI || u.kind == RunnerUnit::XGMI_REPL) {
        // the final wait orders the next forward after every owner's pushes; only if it runs
        // on the comm stream does the compute stream need the end-of-exchange event
        const bool fin = (int)i == last_xgmi_;
        comm_used |= fin && !on_main;
        issue_xgmi(u, lr_t, fin, xs, flag);
        continue;
      }
      comm_used |= !on_main;
      if (u.kind == RunnerUnit::REDUCE) reduces.push_back(&u);
      else issue(u, lr_t, xs);
    }
    if (!reduces.empty()) issue_reduce_group(reduces, lr_t, xs);
  }
  eng_->flush_tail(st);  // a READY flag no launch took (none in the tuned schedules)
  if (comm_used) {
    TraceRange r("ddl.exchange.join");
    // the next step's forward reads the updated parameters
    HIP_CHECK(hipEventRecord(done_ev_, cs_));
    HIP_CHECK(hipStreamWaitEvent(st, done_ev_, 0));
  }
}

// A non-final micro-batch of an accumulated step (set_accum): its gradient goes into the
// accumulator and nowhere else.  No epoch, READY epoch, comm stream, exchange or update.
void SyncRunner::accumulate(const float* x, const int64_t* labels, int B, uint32_t seed_value,
                            hipStream_t st) {
  if (closed_) throw std::runtime_error("sync runner: accumulate() after close()");
  stage_.accum.expect(false);
  TraceRange step_range("ddl.accumulate");
  upd_launches_ = eng_->update_launches = 0;
  eng_->seed_value = seed_value;
  const MicroBatch mb{x, labels, B, st, kBwdRange};
  run_forward(*eng_, mb);
  run_whole_backward(*eng_, mb);
  stage_.accum.accumulate(g_, st);
}

void SyncRunner::issue_xgmi(const RunnerUnit& u, const float* lr_t, bool final_wait,
                            hipStream_t st, bool gated) {
  XgmiUpdate up;
  const auto& r = u.ranges[0];
  up.rule = opt_.rule;
  up.step = opt_.step_for(lr_t[u.ps]);
  // an owner bucket addresses its runs' state offsets itself (PeerExchange bucket spec)
  const bool own = peer_->owner(u.bucket) >= 0;
  up.m = u.m ? u.m + (own ? 0 : r.state_off) : nullptr;
  up.v = u.v ? u.v + (own ? 0 : r.state_off) : nullptr;
  up.coef = coef_;
  peer_->launch(u.bucket, epoch_, up, final_wait, st, gated);
}

void SyncRunner::peer_selftest_step(hipStream_t st) {
  if (!peer_) throw std::runtime_error("no PeerExchange");
  ++epoch_;
  XgmiUpdate up;
  up.rule.kind = kUpdCopy;
  const int nb = peer_->num_buckets();
  for (int b = 0; b < nb; ++b) peer_->launch(b, epoch_, up, b == nb - 1, st);
}

// Failure detection: RCCL reports remote-peer / network failures
// asynchronously; the trainer polls this between steps and the watchdog aborts the comm (so
// blocked collectives on this rank return and the job can be torn down) on a hang.
std::string SyncRunner::async_error() {
  if (peer_ && peer_->error())
    return "xGMI exchange timed out waiting for a peer (code " + std::to_string(peer_->error()) +
           ")";
  if (!comm_) return std::string();
  ncclResult_t st = ncclSuccess;
  RCCL_CHECK(rccl().CommGetAsyncError(as_comm(comm_), &st));
  if (st == ncclSuccess || st == ncclInProgress) return std::string();
  return rccl().GetErrorString(st);
}

// Orderly teardown: every rank calls this at the same point of its program (after a barrier),
// so a communicator finalisation that synchronises with the peers cannot hang on a rank that
// has not reached it yet; afterwards the destructor has nothing collective left to do.
void SyncRunner::close() {
  if (comm_) {
    HIP_CHECK(hipStreamSynchronize(cs_));
    (void)rccl().CommDestroy(as_comm(comm_));
    comm_ = nullptr;
    --rccl_live_comms();
  }
  // and every stream / event / flag with it: a closed runner holds no hardware queue (the
  // one-card W = 4 rehearsal kept four processes' released runners' queues until GC)
  release();
}

void SyncRunner::abort() {
  if (!comm_) return;
  (void)rccl().CommAbort(as_comm(comm_));
  comm_ = nullptr;
  --rccl_live_comms();
}

// Collective sanity check used before trusting the native path on a multi-GPU job: the RS
// and REDUCE patterns on a known pattern, compared on the host.
bool SyncRunner::selftest(std::string* why) {
  if (!comm_) return world_ <= 1;
  const int64_t c = 1031, n = c * world_;
  float *buf = nullptr, *shard = nullptr;
  HIP_CHECK(hipMalloc(&buf, n * sizeof(float)));
  HIP_CHECK(hipMalloc(&shard, c * sizeof(float)));
  std::vector<float> h(n), out(n);
  auto val = [&](int r, int64_t i) { return (float)((r + 1) * ((i % 13) + 1)); };
  for (int64_t i = 0; i < n; ++i) h[i] = val(rank_, i);
  bool ok = true;
  try {
    HIP_CHECK(hipMemcpy(buf, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    // RS then AG of the reduced chunk: every element = sum_r val(r, i)
    RCCL_CHECK(rccl().ReduceScatter(buf, shard, (size_t)c, ncclFloat32, ncclSum, as_comm(comm_), cs_));
    RCCL_CHECK(rccl().AllGather(shard, buf, (size_t)c, ncclFloat32, as_comm(comm_), cs_));
    HIP_CHECK(hipStreamSynchronize(cs_));
    HIP_CHECK(hipMemcpy(out.data(), buf, n * sizeof(float), hipMemcpyDeviceToHost));
    const float rs = (float)(world_ * (world_ + 1) / 2);
    for (int64_t i = 0; i < n && ok; ++i)
      if (out[i] != rs * (float)((i % 13) + 1)) {
        ok = false;
        if (why) *why = "reduce_scatter/all_gather mismatch at " + std::to_string(i);
      }
    // REDUCE to the last rank, then BROADCAST from it
    const int root = world_ - 1;
    HIP_CHECK(hipMemcpy(buf, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    RCCL_CHECK(rccl().GroupStart());
    RCCL_CHECK(rccl().Reduce(buf, buf, (size_t)n, ncclFloat32, ncclSum, root, as_comm(comm_), cs_));
    RCCL_CHECK(rccl().GroupEnd());
    RCCL_CHECK(rccl().GroupStart());
    RCCL_CHECK(rccl().Broadcast(buf, buf, (size_t)n, ncclFloat32, root, as_comm(comm_), cs_));
    RCCL_CHECK(rccl().GroupEnd());
    HIP_CHECK(hipStreamSynchronize(cs_));
    HIP_CHECK(hipMemcpy(out.data(), buf, n * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n && ok; ++i)
      if (out[i] != rs * (float)((i % 13) + 1)) {
        ok = false;
        if (why) *why = "reduce/broadcast mismatch at " + std::to_string(i);
      }
  } catch (const std::exception& e) {
    ok = false;
    if (why) *why = e.what();
  }
  (void)hipFree(buf);
  (void)hipFree(shard);
  return ok;
}

}  // namespace ddl
