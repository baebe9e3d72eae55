// Where the local updates of a one-worker step go (runner.hip run_riding_backward).  Pure C++ (no
// HIP): the host-side sanitizer program csrc/kernels/tests/update_plan_check.cpp builds it alone.
//
// A piece is a plan-buffer range [lo, hi) with its optimizer state at state_off of PS `ps`'s m / v.
// Pieces adjacent in both the parameter buffer and one PS's state merge.  Per backward segment the
// coalesced pieces become the optimizer tail (tail.h) of the next segment's dual launch when they
// fit one; all of them coalesced are the launches after the backward otherwise.  Same result
// either way: no backward GEMM reads a tensor after its update.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ddl {

constexpr int kTailPieces = 4;    // update pieces of one tail (tail.h UpdTail)
constexpr int kPlanSegments = 4;  // backward segments: head+fc, conv4, conv3, conv2+conv1

struct PlanPiece {
  int64_t lo, hi;       // plan-buffer element range [lo, hi)
  int64_t state_off;    // offset of the range's optimizer state in the PS's m / v
  int ps;
  float* m;             // optimizer state base of the owning PS (never dereferenced here)
  float* v;
  int64_t n() const { return hi - lo; }
};

inline void coalesce_pieces(std::vector<PlanPiece>& v) {
  std::sort(v.begin(), v.end(), [](const PlanPiece& a, const PlanPiece& b) { return a.lo < b.lo; });
  std::vector<PlanPiece> out;
  for (const auto& p : v) {
    if (!out.empty()) {
      PlanPiece& q = out.back();
      if (q.hi == p.lo && q.ps == p.ps && q.m == p.m && q.v == p.v &&
          q.state_off + q.n() == p.state_off) {
        q.hi = p.hi;
        continue;
      }
    }
    out.push_back(p);
  }
  v.swap(out);
}

inline bool aligned16(uintptr_t a) { return (a & 15) == 0; }
// the address of element `off` of the float buffer at `base`
inline uintptr_t float_at(uintptr_t base, int64_t off) { return base + 4 * (uintptr_t)off; }
inline uintptr_t float_at(const float* p, int64_t off) { return float_at((uintptr_t)p, off); }

struct UpdatePlan {
  std::vector<PlanPiece> seg[kPlanSegments];  // coalesced per backward segment
  std::vector<PlanPiece> merged;              // all of them coalesced
  // tail_ok: every segment fits one tail under the momentum rule (w, g, m); tail_v_ok: and every
  // piece has a vector-shaped v, which the Adam rule needs.  Kept apart so that the step decides
  // by the rule at that time.
  bool tail_ok = false, tail_v_ok = false;

  void add(int s, const PlanPiece& p) {
    seg[s].push_back(p);
    merged.push_back(p);
  }
  // segment s's pieces fit one tail by their count
  bool fits(int s) const { return seg[s].size() <= (size_t)kTailPieces; }
  // after the last add(): coalesce; w, g: the addresses of the parameter and gradient buffers
  void finish(uintptr_t w, uintptr_t g) {
    coalesce_pieces(merged);
    tail_ok = tail_v_ok = true;
    for (int s = 0; s < kPlanSegments; ++s) {
      coalesce_pieces(seg[s]);
      tail_ok &= fits(s);
      for (const auto& p : seg[s]) {
        tail_ok &= p.m && p.n() % 4 == 0 && aligned16(float_at(w, p.lo)) &&
                   aligned16(float_at(g, p.lo)) && aligned16(float_at(p.m, p.state_off));
        tail_v_ok &= p.v && aligned16(float_at(p.v, p.state_off));
      }
    }
  }
};

}  // namespace ddl
