// Host-side check of the xGMI slice and inbox plan (xgmi_plan.h), meant for a build with
// -fsanitize=address,undefined: pure C++, no GPU.  Reads plans on stdin, one after another, and
// prints what the planners make of each (or `refused <message>`):
//   geo n per_wg max_slices min_slices
//       -> `geo slice nslice`
//   sync total world rank max_slices repl_bucket nbuckets, then per bucket one line
//   `owner nruns lo hi [state_off] ...` (state offsets only when owner >= 0)
//       -> per bucket `bucket b owner lo c inbox_off slice rslot nslice nruns`, per run of it
//          `run lo n soff voff slice sl0`, `end sl0[nruns]`; then once `final` with the slice counts
//          and owners every record carries for the final wait, and `inbox floats`
//   async total world rank max_slices nps nhosts, then nps lines `lo hi` and one line of hosts
//       -> per PS `shard lo n host slice nslice slice0 inbox_off`, then `inbox floats`
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../xgmi_plan.h"

using namespace ddl;

static bool sync_plan() {
  long long total, owner, lo, hi, so;
  int world, rank, max_slices, repl, nb, nruns;
  if (scanf("%lld %d %d %d %d %d", &total, &world, &rank, &max_slices, &repl, &nb) != 6)
    return false;
  std::vector<XgmiBucketSpec> specs((size_t)nb);
  for (XgmiBucketSpec& sp : specs) {
    if (scanf("%lld %d", &owner, &nruns) != 2) return false;
    sp.owner = (int)owner;
    for (int r = 0; r < nruns; ++r) {
      if (scanf("%lld %lld", &lo, &hi) != 2) return false;
      sp.runs.push_back({lo, hi});
      if (sp.owner >= 0) {
        if (scanf("%lld", &so) != 1) return false;
        sp.state_offs.push_back(so);
      }
    }
  }
  try {
    const XgmiPlan P = plan_buckets(specs, total, world, rank, max_slices, repl);
    bool same = true;  // every record carries the same final-wait tables, and its own identity
    for (size_t b = 0; b < P.rec.size(); ++b) {
      const XgmiLaunch& a = P.rec[b];
      printf("bucket %zu %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d\n", b,
             a.owners[b], a.lo, a.c, a.inbox_off, a.slice, a.rslot, a.nslices[b], a.nruns);
      for (int r = 0; r < a.nruns; ++r)
        printf("run %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d\n", a.run_lo[r],
               a.run_n[r], a.run_soff[r], a.run_voff[r], a.run_slice[r], a.run_sl0[r]);
      if (a.nruns) printf("end %d\n", a.run_sl0[a.nruns]);
      same &= memcmp(a.nslices, P.rec[0].nslices, sizeof(a.nslices)) == 0 &&
              memcmp(a.owners, P.rec[0].owners, sizeof(a.owners)) == 0 && a.bucket == (int)b &&
              a.nbuckets == nb && a.world == world && a.rank == rank && a.repl_bucket == repl &&
              (a.nruns == 0 || a.owner == a.owners[b]);
    }
    printf("final %s", same ? "same" : "DIFFERENT");
    for (int i = 0; i < kXgmiMaxBuckets; ++i)
      printf(" %d:%d", P.rec[0].nslices[i], P.rec[0].owners[i]);
    printf("\ninbox %" PRId64 "\n", P.inbox);
  } catch (const std::invalid_argument& e) {
    printf("refused %s\n", e.what());
  }
  return true;
}

static bool async_plan() {
  long long total, lo, hi;
  int world, rank, max_slices, nps, nhosts, h;
  if (scanf("%lld %d %d %d %d %d", &total, &world, &rank, &max_slices, &nps, &nhosts) != 6)
    return false;
  std::vector<std::pair<int64_t, int64_t>> ranges;
  std::vector<int> hosts;
  for (int p = 0; p < nps; ++p) {
    if (scanf("%lld %lld", &lo, &hi) != 2) return false;
    ranges.push_back({lo, hi});
  }
  for (int p = 0; p < nhosts; ++p) {
    if (scanf("%d", &h) != 1) return false;
    hosts.push_back(h);
  }
  try {
    const AsyncPlan P = plan_async_shards(ranges, hosts, total, world, rank, max_slices);
    for (const AsyncShard& S : P.shard)
      printf("shard %" PRId64 " %" PRId64 " %d %" PRId64 " %d %d %" PRId64 "\n", S.lo, S.n, S.host,
             S.slice, S.nslice, S.slice0, S.inbox_off);
    printf("inbox %" PRId64 "\n", P.inbox);
  } catch (const std::invalid_argument& e) {
    printf("refused %s\n", e.what());
  }
  return true;
}

int main() {
  char what[8];
  while (scanf("%7s", what) == 1) {
    bool ok = false;
    if (strcmp(what, "geo") == 0) {
      long long n, per_wg, max_slices, min_slices;
      ok = scanf("%lld %lld %lld %lld", &n, &per_wg, &max_slices, &min_slices) == 4;
      if (ok) {
        const SliceGeo g = slice_geo(n, per_wg, max_slices, min_slices);
        printf("geo %" PRId64 " %d\n", g.slice, g.nslice);
      }
    } else if (strcmp(what, "sync") == 0) {
      ok = sync_plan();
    } else if (strcmp(what, "async") == 0) {
      ok = async_plan();
    }
    if (!ok) {
      fprintf(stderr, "xgmi_plan_check: malformed input at `%s`\n", what);
      return 2;
    }
  }
  return 0;
}
