// The engine's launch schedule and every decision that turns it into launches: pure C++17, no
// HIP, builds alone (tests/schedule_check.cpp runs it; tests/dispatch_cells.py is its Python
// twin).  engine.hip / engine_impl.h launch what these functions choose.  What runs per step is
// inline integer logic on PODs, no heap: the dispatch path is paid ~17 times a step.
#pragma once
#include <stdint.h>

namespace ddl {

// GEMM-shaped ops, in SURVEY.md §2.6 order.  Index into Schedule::splits / Schedule::cfg.
enum Op {
  OP_CONV1_FWD = 0, OP_CONV2_FWD, OP_CONV3_FWD, OP_CONV4_FWD, OP_FC1_FWD, OP_FC2_FWD,
  OP_FC2_DGRAD, OP_FC2_WGRAD, OP_FC1_DGRAD, OP_FC1_WGRAD,
  OP_CONV4_DGRAD, OP_CONV4_WGRAD, OP_CONV3_DGRAD, OP_CONV3_WGRAD,
  OP_CONV2_DGRAD, OP_CONV2_WGRAD, OP_CONV1_WGRAD,
  OP_COUNT
};

// The block tiles selectable per op at run time: (id, BM, BN, BK, WM, WN, V), the template
// arguments of gemm.h TileCfg / launch_gemm.  Multi-wave blocks share each staged operand tile
// between waves (half the L1/L2 bytes per MFMA of one-wave 32x32 blocks at 64x64), at one barrier
// per K tile.
#define TILE_TRAIN(X)                                                                             \
  X(0, 64, 64, 32, 1, 1, 0)  /* 1 wave 64x64 */                                                   \
  X(1, 128, 64, 32, 2, 1, 0) /* 2 waves of 64x64 */                                               \
  X(2, 64, 32, 32, 1, 1, 0)                                                                       \
  X(3, 32, 32, 32, 1, 1, 0)                                                                       \
  X(4, 32, 64, 32, 1, 1, 0)                                                                       \
  X(5, 32, 32, 16, 1, 1, 0)  /* software-pipelined main loop (gemm.h GemmTile::PIPE) */           \
  X(6, 64, 64, 32, 2, 2, 0)  /* 4 waves of 32x32 sharing one LDS-staged 64x64 block tile */       \
  X(7, 64, 32, 32, 2, 1, 0)  /* 2 waves of 32x32 along M */                                       \
  X(8, 32, 64, 32, 1, 2, 0)  /* 2 waves of 32x32 along N */
// eval-only (conv forward ops at 10k-row test-set chunks; no split-K, so only instantiated for
// those ops)
#define TILE_EVAL(X)                                                                              \
  X(9, 128, 128, 32, 2, 2, 0)  /* 2x2 waves of 64x64 */                                           \
  X(10, 128, 64, 32, 2, 2, 0)  /* 2x2 waves of 64x32 */                                           \
  X(11, 256, 64, 32, 4, 1, 0)  /* 4x1 waves of 64x64 */                                           \
  X(12, 128, 128, 32, 4, 1, 0) /* 4x1 waves of 32x128 */
// the one-wave 32x32x32 tile on v_mfma_f32_16x16x4_f32 with LDS-DMA staging (gemm.h
// GemmTile::mainloop_dma16): CFG_MF16
#define TILE_MF16(X) X(14, 32, 32, 32, 1, 1, 1)
#define TILE_ALL(X) TILE_TRAIN(X) TILE_EVAL(X) TILE_MF16(X)

constexpr int NUM_TILE_CFGS = 9;        // configs 0-8: every op
constexpr int NUM_EVAL_TILE_CFGS = 13;  // configs 9-12: the eval forward of conv2-4
// 32x32 one-wave tiles with the K range split over the waves of ONE workgroup (gemm.h
// gemm_kwave_kernel; `splits` picks 4 / 8 / 16 waves)
constexpr int CFG_KWAVE = 13;
constexpr int CFG_MF16 = 14;
// the K-wave launch on 16-row tiles (kwave16.h gemm_kw16_kernel; `splits` picks 4 / 8 / 16 waves)
constexpr int CFG_KW16 = 15;
// (configs 16-20 — one-wave multi-fragment LDS-DMA tiles and the 32x32 ring tiles — were
// measured in round 5, never won a launch and were removed: docs/DESIGN.md)

// Which op has an instantiation of which config, as bit sets over the ops (engine_impl.h holds
// the three special configs against layers.h KWaveOK / Mf16OK / KW16OK at compile time): the fc
// forwards and data gradients; conv2-4's forward, data and weight gradient (the halo-layout
// convolutions whose 16-byte gathers are the DMA sources); the fc forwards; conv2-4's forward
constexpr uint32_t kKw16Ops = 1u << OP_FC1_FWD | 1u << OP_FC2_FWD;
constexpr uint32_t kKWaveOps = kKw16Ops | 1u << OP_FC2_DGRAD | 1u << OP_FC1_DGRAD;
constexpr uint32_t kEvalTileOps = 1u << OP_CONV2_FWD | 1u << OP_CONV3_FWD | 1u << OP_CONV4_FWD;
constexpr uint32_t kMf16Ops = kEvalTileOps | 0x3fu << OP_CONV4_DGRAD;  // ops 10-15
constexpr bool op_has_cfg(int op, int cfg, bool train) {
  if (op < 0 || op >= OP_COUNT || cfg < 0) return false;
  if (cfg < NUM_TILE_CFGS) return true;
  const uint32_t ops = cfg < NUM_EVAL_TILE_CFGS ? (train ? 0u : kEvalTileOps)
                       : cfg == CFG_KWAVE       ? kKWaveOps
                       : cfg == CFG_MF16        ? kMf16Ops
                       : cfg == CFG_KW16        ? kKw16Ops
                                                : 0u;
  return (ops >> op) & 1;
}
// The config that really runs: one the op has no instantiation of falls back, silently, to the
// one-wave 32x32 tile.  (conv2-4's eval forward sends every config past the training tiles to
// its large-tile switch, whose default is tile 12: the three special configs run that there.)
constexpr int effective_cfg(int op, int cfg, bool train) {
  if (!train && cfg >= NUM_EVAL_TILE_CFGS && op_has_cfg(op, NUM_TILE_CFGS, false)) return 12;
  return op_has_cfg(op, cfg, train) ? cfg : 3;
}
// set_cfg / set_eval_cfg accept a config the op has, or a special one (which then falls back)
constexpr bool cfg_accepted(int op, int cfg, bool train) {
  return op_has_cfg(op, cfg, train) || cfg == CFG_KWAVE || cfg == CFG_MF16 || cfg == CFG_KW16;
}
// dual launches are instantiated for the one-wave configs: 32x32 (3), 32x32 BK 16 pipelined (5)
// and the 16x16x4 tile (CFG_MF16) (the register-staged one-wave 64x64 / 32x64 tiles, 180-230
// VGPRs, never won a dual launch in the real-step tuner)
constexpr bool one_wave_cfg(int c) { return c == 3 || c == 5 || c == CFG_MF16; }

struct Schedule {
  int cfg[OP_COUNT];
  int eval_cfg[OP_COUNT];  // tile configs of the no-split eval forward (train = false)
  int splits[OP_COUNT];
  int wide[OP_COUNT];      // per op: z > wide[op] -> separate wide reduce (mode 2), else the
                           // in-launch last-arriver reduction (mode 1)
  int wide_thr = 1;        // default split count above which the separate wide reduce is used
  bool dual = true;        // single stream: dgrad + wgrad of a layer in one launch
  // bit op: that dual launch dispatches its second problem first.  conv2's (weight gradient
  // split 32 ways, the longer pole) measured 0.3663 -> 0.3650 ms/step; conv4's / conv3's worse
  // (their data gradients are the longer poles; conv4's stream-K loses its XCD-major numbering).
  int dual_bfirst = 1 << OP_CONV2_DGRAD | 1 << OP_CONV3_DGRAD;
  int dual_order(int op) const { return (dual_bfirst >> op) & 1; }
  // weight-gradient GEMMs on a second stream.  Off by default: a cross-queue event wait costs
  // tens of microseconds of GPU idle on MI355X/ROCm (step timelines), more than the overlap
  // gains; dgrad/wgrad concurrency comes from fused dual-problem launches instead.
  bool concurrent = false;
  // conv1 forward on the direct LDS-staged kernel (conv1.hip) instead of the GEMM engine's
  // gather-bound K = 25 launch
  bool conv1_direct = true;
  // conv1's weight gradient on the direct kernel with its in-launch reduce (conv1.h), riding
  // with conv2's weight-gradient reduce, instead of the GEMM launch + wide reduce launch
  bool conv1_wgrad_direct = true;
  // the fc backward's packed launches leave the fc weight gradients to the conv4 dual launch
  // (engine_impl.h FcWgradAux); false: they stay in the packs
  bool fc_wgrad_defer = true;
  // fc2 forward's split-K partials reduced by the head kernel (the step's forward with
  // defer_fc2, one-wave 32x32 split-K in mode 2): one launch fewer per step
  bool fc2_in_head = true;
  bool eval_kmap2 = true;  // eval forward: conv2 on the tap-skipping K map
  static Schedule defaults();  // the tuned schedule; reads no environment
};

inline Schedule Schedule::defaults() {
  // {tile config, split-K} per op: whole-step coordinate-descent tune
  // (scripts/step_tune.py over the scripts/op_bench.py per-op sweep) on one MI355X, batch 100,
  // single-stream backward with dual dgrad+wgrad launches: fwd+bwd 367 us (was 449 us)
  // (round 2, after the halo layout and the batch-minor weight-gradient enumeration: conv2
  // weight gradient on the basic BK 32 loop instead of the pipelined BK 16 one, 342.8 ->
  // 336.5 us, profiles/r2_runner_tune_halo.log)
  // fc1 forward on the K-wave launch (8 waves per workgroup, LDS reduction, no reduce launch):
  // 313.4 -> 310.6 us (profiles/r2_runner_tune_kwave.log); fc1 data gradient as the K-wave
  // half of one packed launch with its weight gradient (gemm_pack_kernel, 4 waves), instead
  // of the one-wave dual launch + wide reduce: 308.7 -> 304.4 us (profiles/r2_runner_tune_pack.log)
  // (round 3, after the direct conv1 kernels: fc2 data gradient on the K-wave half of a packed
  // launch with its weight gradient, like fc1's: 292.8 -> 291.5 us, profiles/r3_runner_tune.log)
  // (round 5, scripts/sched_ab.py on one MI355X, 5 alternating rounds of 300 steps: conv4
  // weight gradient and conv2 data gradient on the 16x16x4 MFMA tile (config 14), conv4 weight
  // gradient split 8: 295.3 -> 293.0 us, profiles/r5_sched_ab_mf16.log; then conv3 weight
  // gradient on config 14 too: 293.5 -> 292.7 us, profiles/r5_sched_ab_conv3w.log — conv2's
  // weight gradient on it loses 6 us)
  // (round 6: fc1's and fc2's forwards on the 16-row K-wave launch, 8 waves — fc2 then writes h2
  // itself and the head reads it instead of fc2's split-K partials: 260.7-261.0 -> 259.1-259.4
  // us/step, 4 interleaved rounds, profiles/r6_sched_ab_kw16.log)
  constexpr int defc[OP_COUNT] = {3, 3, 3, 3, CFG_KW16, CFG_KW16, CFG_KWAVE, 5, CFG_KWAVE, 5,
                                  3, CFG_MF16, 3, CFG_MF16, CFG_MF16, 3, 3};
  // (re-tuned in the real step with scripts/sched_ab.py after the compact 52-row conv3
  // enumeration and the wgrad row decode: conv3 forward split 4 + in-launch reduce instead of
  // stream-K 3072 workers, 372.4 -> 369.5 us; conv4 weight gradient split 4 instead of 8,
  // 370.5 -> 368.0 us; conv4 data gradient 2560 stream-K workers and conv3 weight gradient
  // split 12, 365.2 -> 362.3 us)
  // (round 2, with the tap-skipping K maps of conv3/conv4: conv4 data gradient split-K 4 with
  // a separate reduce instead of stream-K over the full K, 322.2 -> 313.3 us,
  // profiles/r2_runner_tune_kmap.log)
  // (round 3, conv forwards on the LDS-DMA main loop: conv2 / conv3 / conv4 forward split-K
  // 3 / 3 / 6 instead of 2 / 4 / 8, 302.5 -> 299.0 us fwd+bwd, scripts/sched_ab.py
  // --splits-variants, profiles/r3_sched_ab_ldsdma.log)
  // (round 6, after the row-wise data-gradient epilogues made the last arriver cheap: conv4's
  // data gradient split-K 5 with the in-launch reduce instead of 4 + the separate wide reduce,
  // conv3's split-K 5 instead of 8, and the conv3 dual dispatching its weight-gradient blocks
  // first (dual_bfirst): 279.2 -> 267.7 us/step, scripts/sched_ab.py,
  // profiles/r6_sched_ab_grid.log; then conv2's weight gradient split-K 48 instead of 32 and
  // conv4's 6 instead of 8: 267.2 -> 264.8, profiles/r6_sched_ab_wgrad.log; conv4's forward
  // split-K 5 instead of 6 once the last arriver sums its partials in one batched round per 4:
  // 264.4 -> 262.9, profiles/r6_runner_tune.log, r6_sched_ab_zb.log)
  constexpr int defs[OP_COUNT] = {1, 3, 3, 5, 8, 8, 4, 1, 4, 1, 5, 6, 5, 12, 4, 48, 1024};
  // split-K reduce in-launch (last arriver) for these ops, separate wide-reduce kernel otherwise
  constexpr bool inl[OP_COUNT] = {0, 1, 1, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0};
  Schedule s;
  for (int op = 0; op < OP_COUNT; ++op) {
    s.cfg[op] = s.eval_cfg[op] = defc[op];
    s.splits[op] = defs[op];
    s.wide[op] = inl[op] ? (1 << 20) : 1;
  }
  // eval forward at 10k-row chunks (scripts/eval_sweep.py, after the compact conv3 rows):
  // conv2-4 on 4-wave 64x64 blocks, full test-set eval 6.76 -> 6.66 ms (106 TF); round 2:
  // conv3 on the eval-only 128x128 block (2x2 waves of 64x64), 6.62 -> 6.53 ms (108 TF) —
  // the larger eval tiles (9-12) gain at most 1.4 %, so the eval is bound by the main loop,
  // not by tile shape (profiles/r2_eval_sweep_big_tiles.log)
  // round 3 (scripts/eval_sweep.py on the current build, profiles/r3_eval_sweep.log): the
  // one-wave 64x64 tile (4 fragments per wave, no LDS sharing between waves) for conv2-4,
  // full test-set eval 5.04 -> 4.64 ms
  s.eval_cfg[OP_CONV2_FWD] = s.eval_cfg[OP_CONV3_FWD] = s.eval_cfg[OP_CONV4_FWD] = 0;
  return s;
}

// The backward segments: (data-gradient op, weight-gradient op) of each layer of a segment, in launch order, and the op
// that follows the last pair (conv1's weight gradient; -1: none)
struct OpPair { int dgrad, wgrad; };
struct Segment { int npairs; OpPair pair[2]; int then; };
constexpr int kSegments = 4;
constexpr Segment kSegment[kSegments] = {
    {2, {{OP_FC2_DGRAD, OP_FC2_WGRAD}, {OP_FC1_DGRAD, OP_FC1_WGRAD}}, -1},
    {1, {{OP_CONV4_DGRAD, OP_CONV4_WGRAD}, {-1, -1}}, -1},
    {1, {{OP_CONV3_DGRAD, OP_CONV3_WGRAD}, {-1, -1}}, -1},
    {1, {{OP_CONV2_DGRAD, OP_CONV2_WGRAD}, {-1, -1}}, OP_CONV1_WGRAD}};

// The run-time choices of a backward segment's launches, counted on the host where each commits
// to its launches (Engine::branch_hits; tests prove with them that a schedule reached the branch
// it was written for: configs fall back silently).
enum Branch {
  // an fc pair (data + weight gradient of fc2 / fc1): the packed launch with the weight gradient
  // left to the conv4 dual launch, the packed launch that keeps it, the one-wave dual launch,
  // back to back
  BR_FC_PACK_DEFERRED = 0, BR_FC_PACK_KEPT, BR_FC_DUAL, BR_FC_BACK_TO_BACK,
  // conv4's pair: the dual launch with the deferred fc weight gradients (FcWgradAux) or with the
  // optimizer tail alone (TailAux); back to back with fc weight gradients left to flush_fc_wgrad,
  // or with none pending
  BR_CONV4_DUAL_FC_WGRAD, BR_CONV4_DUAL_TAIL, BR_CONV4_BACK_TO_BACK_FLUSH, BR_CONV4_BACK_TO_BACK,
  BR_CONV3_DUAL, BR_CONV3_BACK_TO_BACK,
  // conv2's pair inside the unfused sequence of segment 3
  BR_CONV2_DUAL, BR_CONV2_BACK_TO_BACK,
  // segment 3 fused (dual_then_b): conv1's direct kernel with conv2's reduce riding in it or with
  // none pending; the reduce fused with conv1's GEMM (launch_reduce_with_gemm) or its refusal
  // (launch_reduce, then run_op).  Which of the four is known only once the launch is planned.
  BR_SEG3_DIRECT_REDUCE, BR_SEG3_DIRECT, BR_SEG3_REDUCE_GEMM, BR_SEG3_REDUCE_REFUSED,
  BR_SEG3_UNFUSED,            // run_dual_inst + run_op
  BR_TAIL_STANDALONE,         // flush_tail issued update launches of its own
  BR_TAIL_CONSUMED,           // a launch took the pending tail (dual, pack, FcWgradAux)
  BR_CONCURRENT,              // a segment in the two-stream mode
  BR_COUNT
};
inline const char* branch_name(int b) {
  constexpr const char* names[BR_COUNT] = {
      "fc_pack_deferred", "fc_pack_kept", "fc_dual", "fc_back_to_back",
      "conv4_dual_fc_wgrad", "conv4_dual_tail", "conv4_back_to_back_flush", "conv4_back_to_back",
      "conv3_dual", "conv3_back_to_back", "conv2_dual", "conv2_back_to_back",
      "seg3_direct_reduce", "seg3_direct", "seg3_reduce_gemm", "seg3_reduce_refused",
      "seg3_unfused", "tail_standalone", "tail_consumed", "concurrent"};
  return b >= 0 && b < BR_COUNT ? names[b] : "";
}

// Ops oa and ob (independent) in one launch if both use one-wave tiles, else back to back.  oa on
// the K-wave config (fc data gradients) with ob on a one-wave 32x32 config: one packed launch
// (gemm.h gemm_pack_kernel; ob's tiles run BK 32 there).  fc only: the packed launch runs ob's
// tiles unsplit over the raw K range, which the conv weight gradients' tap-window K maps do not
// support; a conv pair with a K-wave op runs back to back.
enum PairKind { PAIR_PACK, PAIR_DUAL, PAIR_BACK_TO_BACK };
struct PairChoice {
  PairKind kind;
  int ca, cb;    // PAIR_DUAL: the one-wave configs that run (effective_cfg)
  bool defers;   // PAIR_PACK: the weight gradient is left to the conv4 dual launch
};
constexpr bool is_fc_pair(int oa) { return oa == OP_FC2_DGRAD || oa == OP_FC1_DGRAD; }
inline PairChoice choose_pair(const Schedule& s, int oa, int ob) {
  const int ca = s.cfg[oa], cb = s.cfg[ob];
  if (s.dual && is_fc_pair(oa) && ca == CFG_KWAVE && (cb == 3 || cb == 5))
    return {PAIR_PACK, ca, cb, s.fc_wgrad_defer};
  if (s.dual && one_wave_cfg(ca) && one_wave_cfg(cb))
    return {PAIR_DUAL, effective_cfg(oa, ca, true), effective_cfg(ob, cb, true), false};
  return {PAIR_BACK_TO_BACK, ca, cb, false};
}
// fc_wgrad_pending: deferred fc weight gradients wait for conv4's pair
constexpr Branch pair_branch(int oa, PairKind k, bool defers, bool fc_wgrad_pending) {
  if (is_fc_pair(oa))
    return k == PAIR_PACK   ? (defers ? BR_FC_PACK_DEFERRED : BR_FC_PACK_KEPT)
           : k == PAIR_DUAL ? BR_FC_DUAL
                            : BR_FC_BACK_TO_BACK;
  if (oa == OP_CONV4_DGRAD)
    return k == PAIR_DUAL ? (fc_wgrad_pending ? BR_CONV4_DUAL_FC_WGRAD : BR_CONV4_DUAL_TAIL)
                          : (fc_wgrad_pending ? BR_CONV4_BACK_TO_BACK_FLUSH : BR_CONV4_BACK_TO_BACK);
  if (oa == OP_CONV3_DGRAD) return k == PAIR_DUAL ? BR_CONV3_DUAL : BR_CONV3_BACK_TO_BACK;
  return k == PAIR_DUAL ? BR_CONV2_DUAL : BR_CONV2_BACK_TO_BACK;
}
// does the pair's launch carry the pending optimizer tail?  (fc2's launches carry fc3's weight
// gradient instead, and a pair back to back has no launch with aux blocks: the tail is flushed)
constexpr bool pair_takes_tail(int oa, PairKind k) {
  return k != PAIR_BACK_TO_BACK && oa != OP_FC2_DGRAD;
}

// Segment 3 fused (engine_impl.h dual_then_b: the conv2 dual launch, which takes the pending tail,
// then conv1's weight gradient sharing a launch with conv2's weight-gradient reduce) or unfused
// (the pair as choose_pair says, then conv1's weight gradient).  Fused is instantiated for conv2's
// data gradient on 3 or CFG_MF16 (not the pipelined 5), its weight gradient on any one-wave
// config and conv1's weight gradient on 32x32 split-K.
struct Seg3Choice { bool fused; int ca, cb; };  // ca, cb: as PairChoice's
inline Seg3Choice choose_seg3(const Schedule& s) {
  constexpr Segment g = kSegment[3];
  const int oa = g.pair[0].dgrad, ob = g.pair[0].wgrad;
  const int ca = s.cfg[oa], cb = s.cfg[ob];
  if (!s.dual || !one_wave_cfg(ca) || ca == 5 || !one_wave_cfg(cb) || s.cfg[g.then] != 3)
    return {false, ca, cb};
  return {true, effective_cfg(oa, ca, true), effective_cfg(ob, cb, true)};
}

}  // namespace ddl
