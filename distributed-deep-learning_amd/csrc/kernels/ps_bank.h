// The parameter servers one process hosts and the optimizer they step with: the one home of what
// AsyncService (xgmi_async.hip), RcclAsync (rccl_async.hip) and AsyncRunner's in-line mode
// (async_runner.hip) share.  Pure C++ (no HIP): the host-side sanitizer program
// csrc/kernels/tests/ps_bank_check.cpp builds it alone.
#pragma once
#include <stdint.h>

#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "update.h"

namespace ddl {

constexpr int kAsyncMaxPs = 64;

// An optimizer as a site holds it: the rule, and the step size's operands exactly as handed in.
// TF1 Adam's lr_t can differ in its last bit with the width of lr, b1 and b2 (docs/DESIGN.md), so
// a site names its convention by the constructor it calls.  The rule's c1 / c2 come from the
// float32 betas under both.  Refused: an unknown kind, a negative decay, Nesterov without momentum.
struct OptimSpec {
  UpdRule rule;
  double lr = 1e-4, b1 = 0.9, b2 = 0.999;

  // true doubles, as ops/adam.py adam_coeffs: RcclAsync, and every site that is handed its lr_t
  static OptimSpec from_doubles(int kind, double lr, double b1, double b2, float eps, float mu,
                                float scale, float decay = 0.f, bool nesterov = false) {
    if (kind < kUpdAdam || kind > kUpdCopy) throw std::invalid_argument("rule kind");
    if (!(decay >= 0.f)) throw std::invalid_argument("negative weight decay");
    if (nesterov && kind != kUpdMomentum)
      throw std::invalid_argument("Nesterov needs the momentum rule");
    OptimSpec s;
    s.rule = UpdRule(kind, (float)b1, (float)b2, eps, mu, scale, decay, nesterov);
    s.lr = lr, s.b1 = b1, s.b2 = b2;
    return s;
  }
  // lr, b1 and b2 rounded to float32, then widened: AsyncService and the in-line runner.  (Through
  // volatile floats: g++ 11 -O3 has vectorized the plain casts of lr and b1 away in one caller.)
  static OptimSpec from_float32(int kind, double lr, double b1, double b2, float eps, float mu,
                                float scale, float decay = 0.f, bool nesterov = false) {
    volatile float l = (float)lr, x1 = (float)b1, x2 = (float)b2;
    return from_doubles(kind, l, x1, x2, eps, mu, scale, decay, nesterov);
  }
  // the step size of step t (1-based) of a PS that keeps its own counter
  float step_at(int64_t t) const {
    return rule.kind == kUpdMomentum ? (float)lr : adam_step_size(lr, b1, b2, t);
  }
  // the same where the caller holds Adam's lr_t already
  float step_for(float lr_t) const { return rule.kind == kUpdMomentum ? (float)lr : lr_t; }
};

struct AsyncPsState {            // one hosted PS
  int ps;
  float* params;                 // the PS's private parameter copy
  float* m;
  float* v;
  int64_t t;                     // its step counter (advanced once per arrival)
};

class PsBank {
 public:
  struct Step {
    int64_t t;
    float step;
  };
  PsBank() = default;
  // ps: the hosted states, ids in [0, num_ps), each once; `tag` prefixes the error messages
  PsBank(const char* tag, const std::vector<AsyncPsState>& ps, int num_ps, const OptimSpec& spec,
         bool provenance)
      : tag_(tag), ps_(ps), slot_(num_ps > 0 ? num_ps : 0, -1), spec_(spec), keep_(provenance) {
    if (ps.size() > (size_t)kAsyncMaxPs) throw std::invalid_argument(tag_ + ": too many PS");
    for (size_t i = 0; i < ps.size(); ++i) {
      const AsyncPsState& s = ps[i];
      if (s.ps < 0 || s.ps >= num_ps || slot_[s.ps] >= 0 || !s.params || !s.m ||
          (spec.rule.kind == kUpdAdam && !s.v))
        throw std::invalid_argument(tag_ + ": PS state");
      slot_[s.ps] = (int)i;
    }
  }
  const OptimSpec& spec() const { return spec_; }
  std::vector<AsyncPsState>& states() { return ps_; }  // in the order given
  AsyncPsState& at(int ps) { return ps_[slot_of(ps)]; }
  int64_t t(int ps) const {  // lock-free: also read while a service thread advances it
    return __atomic_load_n(&ps_[slot_of(ps)].t, __ATOMIC_ACQUIRE);
  }
  void set_t(int ps, int64_t t) {
    if (t < 0) throw std::invalid_argument(tag_ + ": negative step counter");
    __atomic_store_n(&at(ps).t, t, __ATOMIC_RELEASE);
  }
  // one apply_gradients of a hosted PS: its next step and that step's size
  Step advance(AsyncPsState& st) const {
    const int64_t t = __atomic_add_fetch(&st.t, 1, __ATOMIC_ACQ_REL);
    return Step{t, spec_.step_at(t)};
  }
  void keep_provenance(bool on) { keep_ = on; }
  void record(int64_t worker, int64_t ps, int64_t round, int64_t t) {
    if (keep_) prov_.push_back({worker, ps, round, t});
  }
  // (worker, ps, round, PS step) per recorded apply, in call order
  const std::vector<std::array<int64_t, 4>>& provenance() const { return prov_; }

 private:
  size_t slot_of(int ps) const {
    if (ps < 0 || ps >= (int)slot_.size() || slot_[ps] < 0)
      throw std::invalid_argument(tag_ + ": PS " + std::to_string(ps) + " not hosted here");
    return (size_t)slot_[ps];
  }
  std::string tag_;
  std::vector<AsyncPsState> ps_;
  std::vector<int> slot_;        // PS id -> index in ps_ (-1: not hosted)
  OptimSpec spec_;
  bool keep_ = false;
  std::vector<std::array<int64_t, 4>> prov_;
};

}  // namespace ddl
