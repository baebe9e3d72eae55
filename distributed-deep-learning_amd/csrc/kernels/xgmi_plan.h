// The host arithmetic of the xGMI data plane (xgmi.hip, xgmi_async.hip): how a bucket or a PS shard
// is cut into workgroup slices and where its pieces lie in an inbox.  One slice rule, the bucket
// planner behind PeerExchange and the shard planner behind AsyncPeer, with their refusals.  Pure
// C++ (no HIP): the host-side sanitizer program csrc/kernels/tests/xgmi_plan_check.cpp builds it
// alone, and tests/test_xgmi_plan_cpu.py holds it against tests/exchange_reference.py.
#pragma once
#include <stdint.h>
#include <string.h>

#include <stdexcept>
#include <utility>
#include <vector>

#include "ps_bank.h"

namespace ddl {

constexpr int kXgmiMaxPeers = 16;
// flat plans: one bucket per backward segment (<= 8); tensor-granular plans: one OWNER bucket per
// (PS, segment) exchange unit (<= 8 PS x 4 segments)
constexpr int kXgmiMaxBuckets = 32;
constexpr int kXgmiMaxRuns = 8;   // plan-buffer ranges of one owner bucket
#ifndef DDL_XGMI_MAX_SLICES
#define DDL_XGMI_MAX_SLICES 512
#endif
constexpr int kXgmiMaxSlices = DDL_XGMI_MAX_SLICES;
constexpr int kAsyncMaxSlices = 512;

struct XgmiLaunch {              // one bucket's kernel arguments
  int world, rank, bucket, nbuckets, final_wait;
  uint32_t epoch;
  int64_t lo, c, inbox_off, slice;
  int nslices[kXgmiMaxBuckets];
  const float* grads;
  float* m;
  float* v;
  UpdRule rule;                  // the owner-side update (update.h) and its step size
  float step, coef;
  int* err;
  long long timeout_ticks;
  int check;                     // DDL_XGMI_CHECK: per-(bucket, source, slice) inbox checksums
  int repl_bucket;               // the replicated bucket (-1: none)
  int owners[kXgmiMaxBuckets];   // -1: chunk r of the bucket on rank r; >= 0: single owner rank
  // the READY gate ahead of this kernel on the comm stream timed out (host word, or null): the
  // segment's gradients may be incomplete, so the kernel publishes nothing (no pushes, no
  // ARRIVE / DONE words); the peers then time out too and every host raises
  const int* gate_err;
  // owner buckets: the launched bucket's runs (plan-buffer range, element offset in the owner
  // PS's optimizer state, offset in the bucket's concatenation, slice size, first slice)
  int owner, nruns;
  int64_t run_lo[kXgmiMaxRuns], run_n[kXgmiMaxRuns], run_soff[kXgmiMaxRuns];
  int64_t run_voff[kXgmiMaxRuns], run_slice[kXgmiMaxRuns];
  int run_sl0[kXgmiMaxRuns + 1];
  int64_t rslot;                 // the replicated bucket's inbox slot stride (floats)
};
// One bucket of a PeerExchange.  owner < 0: a single plan-buffer range split into W equal chunks,
// chunk r owned by rank r (the flat plan: reduce-scatter form).  owner >= 0: one PS's exchange
// unit of a tensor-granular plan (reference none / contiguous / greedy, lpt; or a flat plan with
// fewer PS than ranks) — every rank pushes the whole unit to its owner, which sums, updates with
// that PS's optimizer state (run r at state_offs[r]) and pushes the parameters to every rank.
struct XgmiBucketSpec {
  std::vector<std::pair<int64_t, int64_t>> runs;
  std::vector<int64_t> state_offs;
  int owner = -1;
};
struct AsyncShard {              // one PS's contiguous range of the flat buffer
  int64_t lo, n, slice, inbox_off;
  int host, nslice;
  int slice0;                    // its first slice in the dense numbering of all PS' slices
};

// The slice rule: n floats over ns = clamp(ceil(n / per_wg), min_slices, max_slices) workgroups,
// each `slice` = ceil(n / ns) rounded up to whole float4; the last slice may be short, and
// rounding may leave fewer than ns slices.
struct SliceGeo {
  int64_t slice;
  int nslice;
};
inline SliceGeo slice_geo(int64_t n, int64_t per_wg, int64_t max_slices, int64_t min_slices) {
  int64_t ns = (n + per_wg - 1) / per_wg;
  if (ns > max_slices) ns = max_slices;
  if (ns < min_slices) ns = min_slices;
  const int64_t slice = ((n + ns - 1) / ns + 3) & ~(int64_t)3;
  return {slice, (int)((n + slice - 1) / slice)};
}

// Every bucket's launch record with its plan-derived fields set (the rest zero: PeerExchange adds
// the pointers, the timeout and the check mode once, and the per-launch fields per launch), and the
// floats of each rank's inbox.  Every rank computes every rank's layout identically.
struct XgmiPlan {
  std::vector<XgmiLaunch> rec;
  int64_t inbox = 0;
};
inline XgmiPlan plan_buckets(const std::vector<XgmiBucketSpec>& buckets, int64_t total, int world,
                             int rank, int max_slices, int repl_bucket) {
  if (world < 1 || world > kXgmiMaxPeers) throw std::invalid_argument("xgmi: world out of range");
  if (rank < 0 || rank >= world) throw std::invalid_argument("xgmi: rank out of range");
  if (buckets.empty() || (int)buckets.size() > kXgmiMaxBuckets)
    throw std::invalid_argument("xgmi: 1..32 buckets");
  if (max_slices < 1 || max_slices > kXgmiMaxSlices)
    throw std::invalid_argument("xgmi: max_slices out of range");
  if (repl_bucket >= (int)buckets.size()) throw std::invalid_argument("xgmi: replicated bucket");
  XgmiPlan P;
  for (size_t bi = 0; bi < buckets.size(); ++bi) {
    const XgmiBucketSpec& sp = buckets[bi];
    const bool repl = (int)bi == repl_bucket;
    XgmiLaunch a;
    memset(&a, 0, sizeof(a));
    a.world = world;
    a.rank = rank;
    a.bucket = (int)bi;
    a.nbuckets = (int)buckets.size();
    a.repl_bucket = repl_bucket;
    a.inbox_off = P.inbox;
    if (sp.owner >= 0) {
      // owner bucket: the runs concatenated; each run sliced on its own (a slice never crosses
      // a run), >= 1024 elements per slice, at most max_slices slices over the whole unit
      if (sp.owner >= world) throw std::invalid_argument("xgmi: bucket owner out of range");
      if (repl) throw std::invalid_argument("xgmi: an owner bucket cannot be replicated");
      if (sp.runs.empty() || (int)sp.runs.size() > kXgmiMaxRuns ||
          sp.state_offs.size() != sp.runs.size())
        throw std::invalid_argument("xgmi: owner bucket needs 1..8 runs with state offsets");
      int64_t n = 0;
      for (size_t r = 0; r < sp.runs.size(); ++r) {
        const int64_t lo = sp.runs[r].first, hi = sp.runs[r].second;
        if (lo < 0 || hi > total || hi <= lo || (hi - lo) % 4 || lo % 4 || sp.state_offs[r] % 4 ||
            sp.state_offs[r] < 0)
          throw std::invalid_argument("xgmi: owner-bucket run out of range or not 16-B shaped");
        n += hi - lo;
      }
      const int64_t per = slice_geo(n, 1024, max_slices, (int64_t)sp.runs.size()).slice;
      a.owner = sp.owner;
      a.nruns = (int)sp.runs.size();
      int sl = 0;
      int64_t voff = 0;
      for (int r = 0; r < a.nruns; ++r) {
        const int64_t rn = sp.runs[r].second - sp.runs[r].first;
        a.run_lo[r] = sp.runs[r].first;
        a.run_n[r] = rn;
        a.run_soff[r] = sp.state_offs[r];
        a.run_voff[r] = voff;
        a.run_slice[r] = per;
        a.run_sl0[r] = sl;
        sl += (int)((rn + per - 1) / per);
        voff += rn;
      }
      a.run_sl0[a.nruns] = sl;
      if (sl > kXgmiMaxSlices) throw std::invalid_argument("xgmi: owner bucket has too many slices");
      a.lo = sp.runs[0].first;
      a.c = n;
      a.slice = per;
      a.nslices[bi] = sl;
      if (n * 4 * world > 0x7fffffffLL) throw std::invalid_argument("xgmi: bucket too large");
      P.inbox += n * world;
    } else {
      if (sp.runs.size() != 1)
        throw std::invalid_argument("xgmi: equal-chunk bucket needs one range");
      const int64_t lo = sp.runs[0].first, hi = sp.runs[0].second;
      if (lo < 0 || hi > total || hi <= lo) throw std::invalid_argument("xgmi: bucket out of range");
      if ((hi - lo) % (repl ? 4 : 4 * world))
        throw std::invalid_argument("xgmi: bucket not divisible by 4W (replicated: by 4)");
      a.lo = lo;
      // equal-chunk buckets: this rank's chunk; the replicated bucket: all of it
      a.c = repl ? hi - lo : (hi - lo) / world;
      // >= 1024 elements (4 KB) per workgroup slice, at most max_slices workgroups
      const SliceGeo g = slice_geo(a.c, 1024, max_slices, 1);
      a.slice = g.slice;
      a.nslices[bi] = g.nslice;
      a.rslot = a.c;
      if (a.c * 4 * world * (repl ? 2 : 1) > 0x7fffffffLL)
        throw std::invalid_argument("xgmi: bucket too large");
      P.inbox += a.c * world * (repl ? 2 : 1);  // replicated: two parity slots per source
    }
    P.rec.push_back(a);
  }
  // what the final wait of any launch needs of every bucket: its slice count and its owner
  for (XgmiLaunch& a : P.rec)
    for (int i = 0; i < kXgmiMaxBuckets; ++i) {
      const bool has = i < (int)buckets.size();
      a.nslices[i] = has ? P.rec[i].nslices[i] : 0;
      a.owners[i] = has ? buckets[i].owner : -1;
    }
  return P;
}

// Every PS's shard descriptor and the floats of this rank's inbox.  The inbox of a host: one
// [W][n] slot block per hosted PS, in PS order (every rank computes every host's layout
// identically, so pushes know where to write).
struct AsyncPlan {
  std::vector<AsyncShard> shard;
  int64_t inbox = 0;
};
inline AsyncPlan plan_async_shards(const std::vector<std::pair<int64_t, int64_t>>& ps_ranges,
                                   const std::vector<int>& ps_host, int64_t total, int world,
                                   int rank, int max_slices) {
  if (world < 1 || world > kXgmiMaxPeers) throw std::invalid_argument("async xgmi: world");
  if (rank < 0 || rank >= world) throw std::invalid_argument("async xgmi: rank");
  if (ps_ranges.empty() || (int)ps_ranges.size() > kAsyncMaxPs ||
      ps_ranges.size() != ps_host.size())
    throw std::invalid_argument("async xgmi: 1..64 PS, one host each");
  if (max_slices < 1 || max_slices > kAsyncMaxSlices)
    throw std::invalid_argument("async xgmi: max_slices");
  AsyncPlan P;
  std::vector<int64_t> off(world, 0);
  int slice0 = 0;
  for (size_t p = 0; p < ps_ranges.size(); ++p) {
    AsyncShard S;
    S.lo = ps_ranges[p].first;
    S.n = ps_ranges[p].second - ps_ranges[p].first;
    S.host = ps_host[p];
    if (S.lo < 0 || S.n <= 0 || S.lo + S.n > total || S.n % 4 || S.lo % 4)
      throw std::invalid_argument("async xgmi: PS range must be a 4-aligned slice of the buffer");
    if (S.host < 0 || S.host >= world) throw std::invalid_argument("async xgmi: PS host");
    // >= 2048 elements (8 KB) per workgroup, at most max_slices workgroups: a 1.6 M-element
    // shard spreads over 512 workgroups (64 left the apply at ~2 TB/s, 41.6 us for the whole
    // model at W = 1, profiles/r4_step_timeline_async_xgmi_w1.txt)
    const SliceGeo g = slice_geo(S.n, 2048, max_slices, 1);
    S.slice = g.slice;
    S.nslice = g.nslice;
    S.slice0 = slice0;
    slice0 += S.nslice;
    if (S.n * 4 * world > 0x7fffffffLL) throw std::invalid_argument("async xgmi: shard too large");
    S.inbox_off = off[S.host];
    off[S.host] += S.n * world;
    P.shard.push_back(S);
  }
  P.inbox = off[rank];
  return P;
}

}  // namespace ddl
