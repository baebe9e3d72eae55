// Host-side check of the hosted-PS bank and its optimizer spec (ps_bank.h), meant for a build
// with -fsanitize=address,undefined: pure C++, no GPU.
//   ps_bank_check steps   reads lines `width lr b1 b2 kind t` (width: f64 = OptimSpec::from_doubles,
//                         f32 = OptimSpec::from_float32) and prints the float32 bits of step_at(t)
//                         in hex, one line per line read
//   ps_bank_check bank    checks the bank: the refusals of malformed specs and state lists,
//                         advance() from two threads, t / set_t, record(), lookup by PS id.
//                         Prints "OK <checks> checks" and returns 0, or the first failures and 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../ps_bank.h"

using namespace ddl;

static int fails = 0, checks = 0;
#define CHECK(c, ...)                 \
  do {                                \
    ++checks;                         \
    if (!(c)) {                       \
      if (fails++ < 10) {             \
        printf("FAIL %s: ", #c);      \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

template <class F>
static bool refused(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static int steps() {
  char width[8];
  double lr, b1, b2;
  int kind;
  long long t;
  while (scanf("%7s %lf %lf %lf %d %lld", width, &lr, &b1, &b2, &kind, &t) == 6) {
    const bool f32 = strcmp(width, "f32") == 0;
    if (!f32 && strcmp(width, "f64") != 0) return 2;
    const OptimSpec s = f32 ? OptimSpec::from_float32(kind, lr, b1, b2, 1e-8f, 0.9f, 1.f)
                            : OptimSpec::from_doubles(kind, lr, b1, b2, 1e-8f, 0.9f, 1.f);
    const float step = s.step_at(t);
    uint32_t bits;
    memcpy(&bits, &step, 4);
    printf("%08" PRIx32 "\n", bits);
  }
  return 0;
}

static int bank() {
  float buf[4] = {};
  float *w = buf, *m = buf + 1, *v = buf + 2;
  const OptimSpec adam = OptimSpec::from_doubles(kUpdAdam, 1e-4, 0.9, 0.999, 1e-8f, 0.f, 1.f);
  const OptimSpec mom = OptimSpec::from_float32(kUpdMomentum, 0.1, 0.0, 0.0, 0.f, 0.9f, 1.f);
  auto make = [&](const std::vector<AsyncPsState>& ps, int num_ps, const OptimSpec& s) {
    return [=] { PsBank b("check", ps, num_ps, s, false); };
  };
  // the spec's refusals, and what it keeps
  CHECK(refused([] { OptimSpec::from_doubles(3, 0.1, 0.9, 0.999, 0.f, 0.f, 1.f); }), "kind 3");
  CHECK(refused([] { OptimSpec::from_doubles(-1, 0.1, 0.9, 0.999, 0.f, 0.f, 1.f); }), "kind -1");
  CHECK(refused([] { OptimSpec::from_float32(kUpdAdam, 0.1, 0.9, 0.999, 0.f, 0.f, 1.f, -1e-3f); }),
        "negative decay");
  CHECK(refused([] {
          OptimSpec::from_doubles(kUpdAdam, 0.1, 0.9, 0.999, 0.f, 0.f, 1.f, 0.f, true);
        }), "Nesterov under Adam");
  CHECK(!refused([] {
          OptimSpec::from_doubles(kUpdMomentum, 0.1, 0.9, 0.999, 0.f, 0.9f, 1.f, 1e-3f, true);
        }), "Nesterov momentum with decay refused");
  CHECK(adam.lr == 1e-4 && adam.b1 == 0.9 && adam.b2 == 0.999, "doubles not kept as handed in");
  CHECK(mom.lr == (double)0.1f, "float32 convention: lr %.17g", mom.lr);
  CHECK(adam.rule.c1 == 1.f - 0.9f && adam.rule.c2 == 1.f - 0.999f, "c1 / c2 from float32 betas");
  CHECK(mom.step_at(7) == 0.1f && mom.step_for(0.5f) == 0.1f, "momentum's step is float32(lr)");
  CHECK(adam.step_for(0.5f) == 0.5f, "Adam's step is the caller's lr_t");
  CHECK(OptimSpec::from_doubles(kUpdCopy, 0.1, 0.9, 0.999, 0.f, 0.f, 1.f).step_for(0.5f) == 0.5f,
        "the copy rule takes lr_t");
  // malformed state lists
  CHECK(refused(make({{2, w, m, v, 0}}, 2, adam)), "id == num_ps accepted");
  CHECK(refused(make({{-1, w, m, v, 0}}, 2, adam)), "negative id accepted");
  CHECK(refused(make({{0, w, m, v, 0}, {0, w, m, v, 0}}, 2, adam)), "duplicate id accepted");
  CHECK(refused(make({{0, nullptr, m, v, 0}}, 2, adam)), "null params accepted");
  CHECK(refused(make({{0, w, nullptr, v, 0}}, 2, adam)), "null m accepted");
  CHECK(refused(make({{0, w, m, nullptr, 0}}, 2, adam)), "null v accepted under Adam");
  CHECK(!refused(make({{0, w, m, nullptr, 0}}, 2, mom)), "null v refused under momentum");
  std::vector<AsyncPsState> many;
  for (int i = 0; i <= kAsyncMaxPs; ++i) many.push_back({i, w, m, v, 0});
  CHECK(refused(make(many, kAsyncMaxPs + 1, adam)), "%d states accepted", kAsyncMaxPs + 1);
  many.pop_back();
  CHECK(!refused(make(many, kAsyncMaxPs, adam)), "%d states refused", kAsyncMaxPs);
  CHECK(!refused(make({}, 0, adam)), "an empty bank refused");

  // advance() from two threads: every t in 1..2N handed out once, each with its own step size
  {
    constexpr int N = 10000;
    PsBank b("check", {{1, w, m, v, 0}}, 2, adam, false);
    std::vector<PsBank::Step> got[2];
    auto run = [&](int k) {
      got[k].reserve(N);
      for (int i = 0; i < N; ++i) got[k].push_back(b.advance(b.at(1)));
    };
    std::thread a(run, 0), c(run, 1);
    a.join();
    c.join();
    CHECK(b.t(1) == 2 * N, "t = %lld after 2 x %d advances", (long long)b.t(1), N);
    std::vector<int> seen(2 * N + 1, 0);
    bool steps_ok = true, rising = true;
    for (int k = 0; k < 2; ++k)
      for (size_t i = 0; i < got[k].size(); ++i) {
        const PsBank::Step s = got[k][i];
        if (s.t >= 1 && s.t <= 2 * N) ++seen[s.t];
        steps_ok &= s.step == adam.step_at(s.t);
        rising &= i == 0 || s.t > got[k][i - 1].t;
      }
    int once = 0;
    for (int t = 1; t <= 2 * N; ++t) once += seen[t] == 1;
    CHECK(once == 2 * N, "%d of %d step numbers handed out exactly once", once, 2 * N);
    CHECK(steps_ok, "a step size that is not step_at(t)");
    CHECK(rising, "a thread saw its own step numbers out of order");
    CHECK(b.provenance().empty(), "log not empty with nothing recorded");
  }
  // t / set_t and their refusals
  {
    PsBank b("check", {{3, w, m, v, 5}, {0, w, m, v, 9}}, 4, adam, false);
    CHECK(b.t(3) == 5 && b.t(0) == 9, "t as constructed");
    b.set_t(3, 1234567890123LL);
    b.set_t(0, 0);
    CHECK(b.t(3) == 1234567890123LL && b.t(0) == 0, "set_t round trip");
    const PsBank::Step s = b.advance(b.at(0));
    CHECK(s.t == 1 && b.t(0) == 1 && s.step == adam.step_at(1), "advance after set_t(0)");
    CHECK(refused([&] { b.set_t(3, -1); }) && b.t(3) == 1234567890123LL, "negative t accepted");
    CHECK(refused([&] { b.set_t(1, 2); }), "set_t of a PS not hosted");
    CHECK(refused([&] { b.t(2); }), "t of a PS not hosted");
    CHECK(refused([&] { b.t(4); }) && refused([&] { b.t(-1); }), "t of an id out of range");
    CHECK(refused([&] { b.at(1); }), "at() of a PS not hosted");
    CHECK(refused([] { PsBank().t(0); }), "t of an empty bank");
  }
  // record(): call order with provenance on, nothing with it off
  {
    PsBank on("check", {{0, w, m, v, 0}}, 1, adam, true);
    PsBank off("check", {{0, w, m, v, 0}}, 1, adam, false);
    for (int i = 0; i < 5; ++i) {
      on.record(i, 0, 10 + i, 100 - i);
      off.record(i, 0, 10 + i, 100 - i);
    }
    CHECK(off.provenance().empty(), "recorded with provenance off");
    CHECK(on.provenance().size() == 5, "%zu records", on.provenance().size());
    for (size_t i = 0; i < on.provenance().size(); ++i) {
      const auto& r = on.provenance()[i];
      CHECK(r[0] == (int64_t)i && r[1] == 0 && r[2] == 10 + (int64_t)i && r[3] == 100 - (int64_t)i,
            "record %zu out of order", i);
    }
    off.keep_provenance(true);
    off.record(1, 0, 2, 3);
    CHECK(off.provenance().size() == 1, "keep_provenance(true) did not take");
  }
  // eight states, ids in reverse order
  {
    float st[8 * 3] = {};
    std::vector<AsyncPsState> ps;
    for (int i = 0; i < 8; ++i)
      ps.push_back({7 - i, st + 3 * i, st + 3 * i + 1, st + 3 * i + 2, 100 + i});
    PsBank b("check", ps, 8, adam, false);
    for (int id = 0; id < 8; ++id) {
      const int i = 7 - id;
      CHECK(b.at(id).ps == id && b.at(id).params == st + 3 * i && b.at(id).m == st + 3 * i + 1 &&
                b.at(id).v == st + 3 * i + 2 && b.t(id) == 100 + i, "lookup of PS %d", id);
      CHECK(b.states()[i].ps == id, "states() not in the order given");
    }
    b.advance(b.at(5));
    for (int id = 0; id < 8; ++id) CHECK(b.t(id) == 100 + (7 - id) + (id == 5), "t of PS %d", id);
  }
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("OK %d checks\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "steps") == 0) return steps();
  if (argc == 2 && strcmp(argv[1], "bank") == 0) return bank();
  fprintf(stderr, "usage: ps_bank_check steps | bank\n");
  return 2;
}
