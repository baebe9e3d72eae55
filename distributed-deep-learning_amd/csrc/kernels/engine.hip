// The CNN step engine: every forward / backward kernel launch of one worker step.
//
// Reference step: sess.run(grads) on the TF runtime, 14 host round trips
// to push, 14 to pull.  Here a training step at one worker is 16 launches on one stream, all
// buffers preallocated (graph-capturable: no malloc, no sync): the forward, the fused loss head
// and four backward segments in which each layer's data- and weight-gradient GEMMs share one
// dual or packed launch that also carries the previous segment's optimizer tail (the last
// segment's update rides in conv1's weight-gradient launch).  The backward is split into
// segments so the host can push a segment's gradients on a side stream while the next segment
// computes (SURVEY.md §5.8 bucket plan).  What each launch is comes from the schedule
// (schedule.h: Schedule, choose_pair, choose_seg3).  The two-stream mode (Schedule::concurrent:
// weight-gradient GEMMs on a second stream, fork/join events per segment) is the A/B option it
// was measured against; it is slower and off by default.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "api.h"
#include "layers.h"
#include "engine_decl.h"

namespace ddl {

Engine::Engine() : sched(Schedule::defaults()) {
  // DDL_EVAL_KMAP2=0: the image-major GEMM; DDL_CONV1_DIRECT=0 / DDL_CONV1_WGRAD_DIRECT=0: the
  // GEMM paths; DDL_FC2_REDUCE_IN_HEAD=0 keeps fc2's separate reduce launch
  sched.eval_kmap2 = env_flag("DDL_EVAL_KMAP2", true);
  sched.conv1_direct = env_flag("DDL_CONV1_DIRECT", true);
  sched.conv1_wgrad_direct = env_flag("DDL_CONV1_WGRAD_DIRECT", true);
  sched.fc2_in_head = env_flag("DDL_FC2_REDUCE_IN_HEAD", true);
}

Engine::~Engine() {
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_join) (void)hipEventDestroy(ev_join);
  if (side) (void)hipStreamDestroy(side);
}

void Engine::init_streams() {
  if (side) return;
  (void)hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
  (void)hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
  (void)hipEventCreateWithFlags(&ev_join, hipEventDisableTiming);
}

void Engine::op_shape(int op, int B, int* M, int* N, int* K) {
  int m = 0, n = 0, k = 0;
  switch (op) {
    case OP_CONV1_FWD: m = ConvFwd<28, 1, 32>::rows(B); n = 32; k = 25; break;
    case OP_CONV2_FWD: m = ConvFwd<14, 32, 64>::rows(B); n = 64; k = 800; break;
    case OP_CONV3_FWD: m = ConvFwd<7, 64, 128>::rows(B); n = 128; k = 1600; break;
    case OP_CONV4_FWD: m = ConvFwd<4, 128, 256>::rows(B); n = 256; k = 3200; break;
    case OP_FC1_FWD: m = B; n = 1024; k = 1024; break;
    case OP_FC2_FWD: m = B; n = 512; k = 1024; break;
    case OP_FC2_DGRAD: m = B; n = 1024; k = 512; break;
    case OP_FC2_WGRAD: m = 1025; n = 512; k = B; break;
    case OP_FC1_DGRAD: m = B; n = 1024; k = 1024; break;
    case OP_FC1_WGRAD: m = 1025; n = 1024; k = B; break;
    case OP_CONV4_DGRAD: m = B * 16; n = 128; k = 6400; break;
    case OP_CONV4_WGRAD: m = 3201; n = 256; k = WgradConv4::k_of(B); break;
    case OP_CONV3_DGRAD: m = B * 49; n = 64; k = 3200; break;
    case OP_CONV3_WGRAD: m = 1601; n = 128; k = WgradConv3::k_of(B); break;
    case OP_CONV2_DGRAD: m = B * 196; n = 32; k = 1600; break;
    case OP_CONV2_WGRAD: m = 801; n = 64; k = WgradConv2::k_of(B); break;
    case OP_CONV1_WGRAD: m = 26; n = 32; k = WgradConv1::padded_k(B); break;
    default: break;
  }
  *M = m; *N = n; *K = k;
}

// float4 partial-slab elements op `op` needs on config c (a K-wave launch reduces in LDS; it is
// sized as the 32x32 tile)
static size_t slab_need(int op, int c, int M, int N, int K, int s) {
  c = effective_cfg(op, c, true);
  switch (c == CFG_KWAVE || c == CFG_KW16 ? 3 : c) {
#define DDL_SLAB(id, bm, bn, bk, wm, wn, v) \
  case id: return gemm_slab_f4<bm, bn, bk, wm, wn>(M, N, K, s);
    TILE_ALL(DDL_SLAB)
#undef DDL_SLAB
    default: return 0;
  }
}

// Largest slab any op needs at any batch up to B.  Not just at B: a split count is K over the
// chunk rounded up to whole K tiles, so it is not monotonic in the batch (conv4's weight
// gradient, split 6: 5 partials at batch 40, 6 at batch 33 and at every batch <= 32, where the
// batch-minor K is padded to 32 images), and a smaller batch on the same engine — a last
// partial batch, a test — would write its extra partials past the slab.
size_t Engine::slab_floats_needed(int B) const {
  size_t mx = 0;
  for (int b = 1; b <= B; ++b)
    for (int op = 0; op < OP_COUNT; ++op) {
      int M, N, K;
      op_shape(op, b, &M, &N, &K);
      const size_t f = 4 * slab_need(op, sched.cfg[op], M, N, K, sched.splits[op]);
      if (f > mx) mx = f;
    }
  return mx;
}

static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// floats per image: p1..p3 and d4..d2 with the 2-pixel zero halo (layers.h kHalo)
static const size_t kActPer[] = {18 * 18 * 32, 11 * 11 * 64, 8 * 8 * 128, 1024, 1024, 512, 16, 1,
                                 512, 1024, 8 * 8 * 256, 11 * 11 * 128, 18 * 18 * 64, 25088};
static const size_t kCodePer[] = {6272, 3136, 2048, 1024};

size_t Engine::workspace_bytes() const {
  const size_t B = (size_t)max_batch;
  size_t f = 0;
  for (size_t p : kActPer) f += al256(4 * B * p);
  f += 2 * al256(4 * slab_floats);
  for (size_t c : kCodePer) f += al256(B * c);
  f += 256;                          // correct counter
  f += 2 * al256(4 * kMaxTickets);   // split-K arrival tickets (two streams)
  return f;
}

void Engine::bind_workspace(void* base) {
  const size_t B = (size_t)max_batch;
  char* p = (char*)base;
  auto take = [&](size_t bytes) { char* r = p; p += al256(bytes); return r; };
  float** acts[] = {&p1, &p2, &p3, &p4, &h1, &h2, &dlog, &loss,
                    &dpre2fc, &dpre1fc, &d4, &d3, &d2, &d1};
  for (int i = 0; i < 14; ++i) *acts[i] = (float*)take(4 * B * kActPer[i]);
  for (int s = 0; s < 2; ++s) {
    scratch[s].slab = take(4 * slab_floats);
    scratch[s].slab_f4 = slab_floats / 4;
  }
  uint8_t** codes[] = {&c1, &c2, &c3, &c4};
  for (int i = 0; i < 4; ++i) *codes[i] = (uint8_t*)take(B * kCodePer[i]);
  correct = (int*)take(256);
  for (int s = 0; s < 2; ++s) {
    scratch[s].tickets = (int*)take(4 * kMaxTickets);
    scratch[s].max_tiles = kMaxTickets;
  }
}

void Engine::run_op(int op, const float* x, int B, const uint32_t* seed, bool train,
                    hipStream_t st, int si) {
  if (op == OP_CONV1_FWD && sched.conv1_direct) {
    launch_conv1_fwd(x, P[0], P[1], p1, train ? c1 : nullptr, B, st);
    return;
  }
  // (the dual path fuses it with conv2's weight-gradient reduce: engine_impl.h dual_then_b)
  if (op == OP_CONV1_WGRAD && sched.conv1_wgrad_direct &&
      conv1_wgrad_fits(B, slab_floats, scratch[si].max_tiles)) {
    launch_conv1_wgrad_only(x, d1, B, G[0], G[1], static_cast<float*>(scratch[si].slab),
                            scratch[si].tickets, st);
    return;
  }
  switch (op) {
#define DDL_RUN(OPC) \
  case OPC: run_op_inst<OPC>(*this, x, B, seed, train, st, si); break;
    DDL_RUN(OP_CONV1_FWD) DDL_RUN(OP_CONV2_FWD) DDL_RUN(OP_CONV3_FWD) DDL_RUN(OP_CONV4_FWD)
    DDL_RUN(OP_FC1_FWD) DDL_RUN(OP_FC2_FWD) DDL_RUN(OP_FC2_DGRAD) DDL_RUN(OP_FC2_WGRAD)
    DDL_RUN(OP_FC1_DGRAD) DDL_RUN(OP_FC1_WGRAD) DDL_RUN(OP_CONV4_DGRAD) DDL_RUN(OP_CONV4_WGRAD)
    DDL_RUN(OP_CONV3_DGRAD) DDL_RUN(OP_CONV3_WGRAD) DDL_RUN(OP_CONV2_DGRAD)
    DDL_RUN(OP_CONV2_WGRAD) DDL_RUN(OP_CONV1_WGRAD)
#undef DDL_RUN
    default: break;
  }
}

// a push / ready-flag tail (tail.h kinds 1, 2) with no launch to ride in
__global__ void __launch_bounds__(64) push_tail_kernel(UpdTail t) { tail_body(t, blockIdx.x); }

void Engine::flush_tail(hipStream_t st) {
  if (tail.kind != 0) {
    if (tail.nblocks > 0)
      hipLaunchKernelGGL(push_tail_kernel, dim3(tail.nblocks), dim3(64), 0, st, tail);
    tail = UpdTail();
    return;
  }
  int launched = 0;
  for (int i = 0; i < tail.npieces; ++i) {
    const UpdPiece& p = tail.p[i];
    launch_update(tail.rule, p.step, p.span(0), p.g, p.n, st);
    launched += p.n > 0;
  }
  update_launches += launched;
  if (launched) hit(BR_TAIL_STANDALONE);
  tail = UpdTail();
}

void Engine::flush_fc_wgrad(const float* x, int B, const uint32_t* seed, hipStream_t st) {
  const int pend = fc_wgrad_pending;
  fc_wgrad_pending = 0;
  if (pend & 1) run_op(OP_FC2_WGRAD, x, B, seed, true, st, 0);
  if (pend & 2) run_op(OP_FC1_WGRAD, x, B, seed, true, st, 0);
}

void Engine::flush_head_wgrad(int B, hipStream_t st) {
  if (!head_wgrad_pending) return;
  launch_head_wgrad(h2, dlog, B, G[12], G[13], st);
  head_wgrad_pending = 0;
}

void Engine::forward(const float* x, int B, const uint32_t* seed, bool train, hipStream_t st,
                     bool defer_fc2) {
  fc2_slab = nullptr;  // (a deferred fc2 reduce nobody took: this forward rewrites h2 anyway)
  fc_wgrad_pending = 0;  // (likewise: their inputs are about to be rewritten)
  for (int op = OP_CONV1_FWD; op < OP_FC2_FWD; ++op) run_op(op, x, B, seed, train, st, 0);
  if (!(train && defer_fc2 && sched.fc2_in_head && !sched.concurrent && run_fc2_deferred(*this, x, B, seed, st)))
    run_op(OP_FC2_FWD, x, B, seed, train, st, 0);
}

void Engine::flush_fc2(const uint32_t* seed, int B, hipStream_t st) {
  if (fc2_slab) run_fc2_reduce(*this, seed, B, st);
}

// The side stream waits for everything enqueued on `st` so far.
void Engine::fork(hipStream_t st) {
  (void)hipEventRecord(ev_fork, st);
  (void)hipStreamWaitEvent(side, ev_fork, 0);
}

// `st` waits for everything enqueued on the side stream so far.
void Engine::join(hipStream_t st) {
  (void)hipEventRecord(ev_join, side);
  (void)hipStreamWaitEvent(st, ev_join, 0);
}

void Engine::wgrad(int op, const float* x, int B, const uint32_t* seed, hipStream_t st) {
  fork(st);
  run_op(op, x, B, seed, true, side, 1);
}

// pair I of segment S (schedule.h kSegment) as one launch or back to back
template <int S, int I>
static void run_pair(Engine& e, const float* x, int B, const uint32_t* seed, hipStream_t st) {
  run_dual_inst<kSegment[S].pair[I].dgrad, kSegment[S].pair[I].wgrad>(e, x, B, seed, st);
}

void Engine::backward_segment(int s, const float* x, const int64_t* labels, int B,
                              const uint32_t* seed, hipStream_t st) {
  if (s < 0 || s >= kSegments) return;
  if (sched.concurrent && side) {  // weight gradients on the side stream (fork/join per segment)
    hit(BR_CONCURRENT);
    flush_tail(st);
    flush_fc2(seed, B, st);
    if (s == 0) {
      launch_head_fwd(h2, P[12], P[13], labels, B, dlog, loss, nullptr, st);
      launch_head_bwd(h2, P[12], dlog, B, seed, seed_value, thr24, inv_keep, G[12], G[13],
                      dpre2fc, st);
    }
    const Segment& g = kSegment[s];
    for (int i = 0; i < g.npairs; ++i) {
      wgrad(g.pair[i].wgrad, x, B, seed, st);
      run_op(g.pair[i].dgrad, x, B, seed, true, st, 0);
    }
    if (g.then >= 0) wgrad(g.then, x, B, seed, st);
    join(st);
    return;
  }
  // single stream: each layer's dgrad + wgrad as one dual launch
  switch (s) {
    case 0:
      // one head launch (per-sample fwd + dlogits + dh2); fc3's dW/db ride in the fc2 dual.
      // With fc2's reduce deferred the head also finishes fc2 (h2 = its reduce + epilogue).
      if (fc2_slab) {
        launch_head_fused_fc2(fc2_slab, fc2_S, fc2_gx, fc2_ntiles, P[11], h2, P[12], P[13],
                              labels, B, seed, seed_value, thr24, inv_keep, dlog, loss,
                              dpre2fc, st);
        fc2_slab = nullptr;
      } else {
        launch_head_fused(h2, P[12], P[13], labels, B, seed, seed_value, thr24, inv_keep, dlog,
                          loss, dpre2fc, st);
      }
      head_wgrad_pending = 1;
      run_pair<0, 0>(*this, x, B, seed, st);
      flush_head_wgrad(B, st);
      run_pair<0, 1>(*this, x, B, seed, st);
      break;
    case 1:
      run_pair<1, 0>(*this, x, B, seed, st);
      flush_fc_wgrad(x, B, seed, st);  // (a conv4 pair that ran back to back took none of them)
      break;
    case 2: run_pair<2, 0>(*this, x, B, seed, st); break;
    default:
      run_dual_then_inst<kSegment[3].pair[0].dgrad, kSegment[3].pair[0].wgrad, kSegment[3].then>(
          *this, x, B, seed, st);
      break;
  }
}

void Engine::eval_count(const float* x, const int64_t* labels, int B, hipStream_t st) {
  forward(x, B, nullptr, false, st);  // (flushes a pending fc2 reduce of a training forward)
  launch_head_fwd(h2, P[12], P[13], labels, B, nullptr, nullptr, correct, st);
}

}  // namespace ddl
