// The optimizer update rule: one definition for every site that applies it.
//
// Host part (plain C++): the rule kinds, the hyper-parameter carrier UpdRule, the parameter /
// state span UpdSpan and TF1 Adam's host-side step size.  Device part (hipcc only): upd1 / upd4,
// the only callers of common.h's adam1 / momentum1, and the load / update / store forms built on
// them.  Every device form takes the kind as a template argument, so a kernel picks its rule
// once (per launch or per block) and its per-element loop holds one rule's code only; the single
// exception is upd4_any, the xGMI owner kernels' per-element switch, kept as those kernels had it.
//
// The step size is NOT part of the rule: it is per piece and per PS (asynchronous PSs keep their
// own step counters).  `step` is TF1's lr_t under Adam and the plain learning rate under momentum.
#pragma once
#include <math.h>
#include <stdint.h>

namespace ddl {

// UpdRule::kind (the values of the Python side's optimizer index)
enum UpdKind : int {
  kUpdAdam = 0,      // TF1 ApplyAdam (optim.hip)
  kUpdMomentum = 1,  // momentum SGD; mu = 0: plain SGD, m left holding the scaled gradient
  kUpdCopy = 2       // w := g, state untouched (the xGMI self-tests)
};

// UpdRule::flags
enum UpdFlag : int {
  kUpdNesterov = 1  // momentum: the step looks ahead, u = mu * m' + g * scale (else u = m')
};

struct UpdRule {
  int kind = kUpdAdam;
  float c1 = 0.f, c2 = 0.f, eps = 0.f;  // 1 - beta1, 1 - beta2, epsilon (Adam)
  float mu = 0.f;                       // momentum
  float scale = 1.f;                    // gradient scale (1/W mean, or 1 for the reference's sum)
  // The two modifiers of a rule (kUpdCopy ignores both); the kind keeps its three values.
  float decay = 0.f;  // decoupled weight decay lr * wd (upd_decay): w -= decay * w ahead of the
                      // rule's own update, with the plain learning rate under Adam too; 0: none
  int flags = 0;      // UpdFlag bits
  UpdRule() = default;
  UpdRule(int kind_, float b1, float b2, float eps_, float mu_, float scale_, float decay_ = 0.f,
          bool nesterov = false)
      : kind(kind_), c1(1.f - b1), c2(1.f - b2), eps(eps_), mu(mu_), scale(scale_),
        decay(decay_), flags(nesterov ? kUpdNesterov : 0) {}
};

// The decay factor of a rule: lr * weight_decay formed in double and rounded once, so every site
// that is given the same two doubles carries the same float.
inline float upd_decay(double lr, double weight_decay) { return (float)(lr * weight_decay); }

// Parameter and optimizer-state pointers of one range.  v is null under every rule but Adam and
// is then neither offset nor touched.
struct UpdSpan {
  float *w = nullptr, *m = nullptr, *v = nullptr;
  UpdSpan at(int64_t off) const { return UpdSpan{w + off, m + off, v ? v + off : nullptr}; }
};

// TF1 Adam's lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) at step t (1-based), in double, as
// ops/adam.py adam_coeffs.  Called by OptimSpec::step_at alone (ps_bank.h), whose two constructors
// fix the operands' width (float32 widened, or true doubles: they can differ in lr_t's last bit).
inline float adam_step_size(double lr, double b1, double b2, int64_t t) {
  return (float)(lr * sqrt(1.0 - pow(b2, (double)t)) / (1.0 - pow(b1, (double)t)));
}

}  // namespace ddl

#ifdef __HIPCC__
#include "common.h"

namespace ddl {

// One element from the raw gradient g.  Both rules take g and the scale apart and pin their
// roundings (common.h), so every site and kernel shape gives the same bits at every scale; so do
// the two modifiers (decoupled weight decay, Nesterov momentum).
template <int KIND>
DDL_DEV void upd1(const UpdRule& r, float step, float& w, float g, float& m, float& v) {
  static_assert(KIND == kUpdAdam || KIND == kUpdMomentum || KIND == kUpdCopy, "update rule");
  if constexpr (KIND == kUpdCopy) {
    w = g;
  } else {
    // Both modifiers are wave-uniform tests of kernel-argument scalars.  The decay must be
    // skipped, not run with a zero factor: fma(-0, w, w) turns w = -0.0 into +0.0.
    if (r.decay != 0.f) decay1(w, r.decay);
    if constexpr (KIND == kUpdAdam) adam1(w, g, r.scale, m, v, step, r.c1, r.c2, r.eps);
    else if (r.flags & kUpdNesterov) nesterov1(w, g, m, step, r.mu, r.scale);
    else momentum1(w, g, m, step, r.mu, r.scale);
  }
}
template <int KIND>
DDL_DEV void upd4(const UpdRule& r, float step, float4& w, const float4& g, float4& m,
                  float4& v) {
  upd1<KIND>(r, step, w.x, g.x, m.x, v.x);
  upd1<KIND>(r, step, w.y, g.y, m.y, v.y);
  upd1<KIND>(r, step, w.z, g.z, m.z, v.z);
  upd1<KIND>(r, step, w.w, g.w, m.w, v.w);
}

// Element i of a span from gradient g: loads and stores only the streams the rule has.
template <int KIND, class I>
DDL_DEV void upd1_at(const UpdRule& r, float step, float* w, float g, float* m, float* v, I i) {
  float W = 0.f, M = 0.f, V = 0.f;
  if constexpr (KIND != kUpdCopy) { W = w[i]; M = m[i]; }
  if constexpr (KIND == kUpdAdam) V = v[i];
  upd1<KIND>(r, step, W, g, M, V);
  w[i] = W;
  if constexpr (KIND != kUpdCopy) m[i] = M;
  if constexpr (KIND == kUpdAdam) v[i] = V;
}
// float4 i of the state from gradient g; the caller holds (and stores) the parameters w
template <int KIND, class I>
DDL_DEV void upd4_state(const UpdRule& r, float step, float4& w, const float4& g, float4* m,
                        float4* v, I i) {
  float4 M = f4zero(), V = f4zero();
  if constexpr (KIND != kUpdCopy) M = m[i];
  if constexpr (KIND == kUpdAdam) V = v[i];
  upd4<KIND>(r, step, w, g, M, V);
  if constexpr (KIND != kUpdCopy) m[i] = M;
  if constexpr (KIND == kUpdAdam) v[i] = V;
}
// the same with the kind read per element (the xGMI owner / replicated kernels and the
// asynchronous apply: one kernel for every rule, so all of them give the same bits)
DDL_DEV void upd4_any(const UpdRule& r, float step, float4& w, const float4& g, float4* m,
                      float4* v, int i) {
  if (r.kind == kUpdAdam) upd4_state<kUpdAdam>(r, step, w, g, m, v, i);
  else if (r.kind == kUpdMomentum) upd4_state<kUpdMomentum>(r, step, w, g, m, v, i);
  else upd4_state<kUpdCopy>(r, step, w, g, m, v, i);
}

}  // namespace ddl
#endif  // __HIPCC__
