// Native asynchronous worker step (SURVEY.md §3.2 worker loop + §3.4 async PS, over the xGMI
// peer-memory data plane of xgmi_async.hip).
//
// Reference worker round (mnist_async_sharding/worker.py:80-95): sess.run(grads), then one
// MPI Send per tensor to its PS, then a blocking Recv per tensor of the parameters that PS
// sends back.  Here one C++ call per step:
//
//   1. the PREVIOUS round's parameters must be in this worker's buffer before the forward that
//      reads them — the reference's blocking pull.  Default: a GPU-side gate, one wave enqueued
//      on the compute stream after the round's last push, polling the round's DONE words; the
//      forward behind it starts as soon as the last apply lands, with no host in between (the
//      host wait + launch cost ~22 us of idle GPU per step, profiles/r4_async_host_latency.txt).
//      The host only checks, bounded, the round before (failure detection).  set_gate(false):
//      the host waits for the round itself before enqueuing the forward.
//      Why the gate cannot deadlock: it blocks the compute stream's hardware queue until every
//      PS has applied this worker's round.  Those applies run on other processes' queues or on
//      this process's service stream, created with HIGH priority — HIP pools hardware queues
//      per priority, so that stream never shares the gated queue as long as the compute stream
//      is not high priority itself (checked once per stream; a high-priority compute stream gets
//      the host wait instead) — and each apply waits for nothing on the GPU (the service issues
//      it after seeing the push posted).  No wait in the chain sits behind the gate, and the
//      gate is bounded (error word, no hang);
//   2. forward, then the four backward segments; segment s's PS shards are pushed by tail blocks
//      of segment s+1's first launch (tail.h kind 1; the last segment's by a push kernel), each
//      block posting its slice on the arrival board in host memory once its payload is
//      acknowledged: no push kernels on the compute stream, no completion events (whose
//      system-scope release cost ~4.6 us of idle compute stream per push), no host thread
//      between a push and its PS host's service.
//
// In-line applies (set_inline; one worker hosting every PS, Adam — the W = 1 default): the
// push / apply / gate chain above costs ~13 us per step on the critical path after the last
// segment (push launch, host scan, apply launch, DONE, gate) against ~3.5 us for an in-line
// Adam (docs/DESIGN.md round 5).  A sole pusher's pushes reach each PS in the order it issues
// them, so applying segment s's shards as Adam tail blocks of segment s+1's first launch (the
// last segment's inside conv1's weight-gradient launch, engine_impl.h dual_then_b) IS the
// arrival-order apply: the same per-PS Adam step (its own counter t, one step per push), the
// same staleness (none, with one worker), and stream order instead of DONE words.
//
// The PS side: each host's AsyncService scans the board in host memory and issues one apply
// per completed push (Adam on the PS's private copy, the new shard stored into the worker's
// buffer, DONE words in the worker's device flags and in shared host memory).  Staleness stays
// one round per worker.
#include <stdlib.h>

#include <cmath>
#include <stdexcept>
#include <string>

#include "api.h"
#include "common.h"
#include "trace.h"

namespace ddl {

static const char* const kBwdRange[AsyncRunner::kSegments] = {"ddl.bwd", "ddl.bwd", "ddl.bwd",
                                                              "ddl.bwd"};

AsyncRunner::AsyncRunner(Engine* eng, AsyncPeer* peer, int world, int rank, int device,
                         const std::vector<int>& seg_of_ps, uint32_t epoch0)
    : eng_(eng), peer_(peer), world_(world), rank_(rank), device_(device), epoch_(epoch0),
      epoch0_(epoch0) {
  const int P = peer->num_ps();
  if ((int)seg_of_ps.size() != P) throw std::invalid_argument("async runner: one segment per PS");
  // (A/B switches: DDL_ASYNC_GATE=0 waits for the round on the host, DDL_ASYNC_TAIL=0 pushes
  // with kernels of their own instead of tail blocks)
  gate_ = env_flag("DDL_ASYNC_GATE", gate_);
  use_tail_ = env_flag("DDL_ASYNC_TAIL", use_tail_);
  for (int p = 0; p < P; ++p) {
    if (seg_of_ps[p] < 0 || seg_of_ps[p] >= kSegments)
      throw std::invalid_argument("async runner: PS segment out of range");
    seg_ps_[seg_of_ps[p]].push_back(p);
  }
}

void AsyncRunner::wait_round(double timeout_s) {
  if (epoch_ == epoch0_) return;  // no round in flight yet
  TraceRange r("ddl.async.worker.pull_wait");
  if (!peer_->wait_done(epoch_, timeout_s))
    throw std::runtime_error("async runner: round " + std::to_string(epoch_) +
                             " did not come back (kernel error code " +
                             std::to_string(peer_->error()) + ")");
}

void AsyncRunner::check_round(uint32_t e, double timeout_s) {
  TraceRange r("ddl.async.worker.pull_check");
  if (!peer_->wait_done(e, timeout_s))
    throw std::runtime_error("async runner: round " + std::to_string(e) +
                             " did not come back (kernel error code " +
                             std::to_string(peer_->error()) + ")");
}

// The previous round's parameters are in place before a forward reads them: the gate enqueued
// at the end of the previous step (the host checks the round before that: it ran before the
// previous forward, so in steady state this returns at once), or a host wait
void AsyncRunner::wait_params(double timeout_s) {
  if (gated_ != 0) {
    if (gated_ - 1 != epoch0_) check_round(gated_ - 1, timeout_s);
  } else {
    wait_round(timeout_s);
  }
}

void AsyncRunner::set_inline(const std::vector<AsyncPsState>& ps, const OptimSpec& opt,
                             bool provenance) {
  const int P = peer_->num_ps();
  if (world_ != 1) throw std::invalid_argument("async runner: in-line applies need one worker");
  if ((int)ps.size() != P) throw std::invalid_argument("async runner: in-line applies need every PS");
  if (opt.rule.kind != kUpdAdam) throw std::invalid_argument("async runner: in-line applies are Adam");
  PsBank bank("async runner: in-line", ps, P, opt, provenance);  // (one state per PS, m and v)
  for (const auto& s : ps) {
    int64_t lo = 0, n = 0;
    int host = -1;
    peer_->shard(s.ps, lo, n, host);
    if (host != rank_) throw std::invalid_argument("async runner: in-line PS hosted elsewhere");
    if (n % 4 || !aligned16(float_at(peer_->params(), lo)) ||
        !aligned16(float_at(peer_->grads(), lo)) || !aligned16(float_at(s.m, 0)) ||
        !aligned16(float_at(s.v, 0)))
      throw std::invalid_argument("async runner: in-line PS buffers must be 16-B aligned");
  }
  bank_ = bank;
  // one piece per PS: its shard with its own m / v, after the segment that completes it
  plan_ = UpdatePlan();
  for (int sg = 0; sg < kSegments; ++sg)
    for (int p : seg_ps_[sg]) {
      int64_t lo = 0, n = 0;
      int host = -1;
      peer_->shard(p, lo, n, host);
      plan_.add(sg, PlanPiece{lo, lo + n, 0, p, bank_.at(p).m, bank_.at(p).v});
    }
  plan_.finish(reinterpret_cast<uintptr_t>(peer_->params()),
               reinterpret_cast<uintptr_t>(peer_->grads()));
  lr_t_.assign(P, 0.f);
  inline_ = true;
}

void AsyncRunner::inline_sync_ps(hipStream_t st) {
  if (!inline_) return;
  for (int p = 0; p < peer_->num_ps(); ++p) {
    int64_t lo = 0, n = 0;
    int host = -1;
    peer_->shard(p, lo, n, host);
    const hipError_t e = hipMemcpyAsync(bank_.at(p).params, peer_->params() + lo,
                                        (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess)
      throw std::runtime_error(std::string("async runner: PS copy: ") + hipGetErrorString(e));
  }
}

void AsyncRunner::step_inline(const MicroBatch& mb) {
  ++epoch_;
  upd_launches_ = eng_->update_launches = 0;
  // one Adam step of each PS's own counter per push (TF1: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t))
  for (int p = 0; p < (int)lr_t_.size(); ++p) {
    const PsBank::Step s = bank_.advance(bank_.at(p));
    lr_t_[p] = s.step;
    bank_.record(rank_, p, epoch_, s.t);
  }
  const LocalUpdates u{&plan_, &bank_.spec(), lr_t_.data(), peer_->params(), peer_->grads()};
  run_forward(*eng_, mb);
  if (stage_.whole()) {
    // the norm (and the mean over the micro-batches) needs the whole backward: no tails; finish
    // the accumulation, clip, then every segment's applies in segment order (the push order of
    // the plain step)
    run_whole_backward(*eng_, mb);
    stage_.finish(grads(), mb.st);
    for (const auto& sp : plan_.seg) upd_launches_ += launch_piece_updates(u, sp, mb.st);
    return;
  }
  // a segment whose shards do not fit one tail is applied by launches of its own
  RidePolicy pol{{}, 0, kTailF4Default, true};
  for (int s = 0; s < kSegments; ++s) pol.rides[s] = plan_.fits(s);
  upd_launches_ += run_riding_backward(*eng_, mb, u, pol);
}

void AsyncRunner::step(const float* x, const int64_t* labels, int B, uint32_t seed,
                       hipStream_t st, double timeout_s) {
  TraceRange step_range("ddl.async.step");
  stage_.accum.expect(true);
  const MicroBatch mb{x, labels, B, st, kBwdRange};
  if (inline_) {
    eng_->seed_value = seed;
    last_st_ = st;
    stepped_ = true;
    step_inline(mb);
    return;
  }
  // (1) the previous round's parameters are in place before the forward: the gate enqueued at
  // the end of the previous step (the host checks the round before that: it ran before the
  // previous forward, so in steady state this returns at once), or a host wait
  wait_params(timeout_s);
  ++epoch_;
  eng_->seed_value = seed;
  run_forward(*eng_, mb);
  // the gate may only sit on a stream that is not high priority, as the service stream is
  // (queried once per stream: a runtime call at the end of the step would sit in the window where
  // this process's service thread launches the round's last apply)
  const bool gate = gate_place_.safe(st, nullptr) && gate_;
  int last = kSegments - 1;
  while (last > 0 && seg_ps_[last].empty()) --last;
  gated_ = 0;
  const bool clip = stage_.whole();
  if (clip) {
    // a clipped (or accumulated) round: the whole backward with no push tails, the mean over the
    // micro-batches, the clip, then the pushes below in segment order (push kernels of their
    // own; the last carries the gate)
    run_whole_backward(*eng_, mb);
    stage_.finish(grads(), st);
  }
  for (int s = 0; s < kSegments; ++s) {
    if (!clip) {
      TraceRange r("ddl.bwd");
      eng_->backward_segment(s, x, labels, B, nullptr, st);  // (takes a pending push tail)
    }
    if (seg_ps_[s].empty()) continue;
    // (2) this segment's shards to their hosts, posted on the board: as tail blocks of the
    // next segment's first launch (flush_tail launches them alone if it takes none), the last
    // segment's by a push kernel
    TraceRange r("ddl.async.worker.push");
    UpdTail t;
    if (!clip && use_tail_ && s + 1 < kSegments && peer_->push_tail(seg_ps_[s], epoch_, t)) {
      eng_->flush_tail(st);
      eng_->tail = t;
    } else {
      eng_->flush_tail(st);
      // the round's last push carries the pull gate as its launch's last block
      const bool with_gate = gate && s == last;
      peer_->push_set(seg_ps_[s], epoch_, 1.f, st, with_gate);
      if (with_gate) gated_ = epoch_;
    }
  }
  eng_->flush_tail(st);
  if (gate && gated_ == 0) {  // (the last push rode as tail blocks: a gate launch of its own)
    peer_->gate(epoch_, st);
    gated_ = epoch_;
  }
}

// A non-final micro-batch of an accumulated round (set_accum): the parameters it reads are the
// previous round's, as the round's final micro-batch will read them; its gradient goes into the
// accumulator.  No round is opened: no board post, push, gate or apply.
void AsyncRunner::accumulate(const float* x, const int64_t* labels, int B, uint32_t seed,
                             hipStream_t st, double timeout_s) {
  TraceRange step_range("ddl.async.accumulate");
  stage_.accum.expect(false);
  if (inline_) {
    last_st_ = st;
    stepped_ = true;
  } else {
    wait_params(timeout_s);
  }
  eng_->seed_value = seed;
  const MicroBatch mb{x, labels, B, st, kBwdRange};
  run_forward(*eng_, mb);
  run_whole_backward(*eng_, mb);
  stage_.accum.accumulate(grads(), st);
}

void AsyncRunner::finish(double timeout_s) {
  if (inline_) {  // the round's applies are on the compute stream
    if (stepped_) {
      const hipError_t e = hipStreamSynchronize(last_st_);
      if (e != hipSuccess)
        throw std::runtime_error(std::string("async runner: finish: ") + hipGetErrorString(e));
    }
    return;
  }
  wait_round(timeout_s);
}

}  // namespace ddl
