// Host-side run of the local-update planner (update_plan.h), meant for a build with
// -fsanitize=address,undefined: pure C++, no GPU.  Reads plans from standard input,
//   plan NAME
//   SEG LO HI PS STATE_OFF        (one line per range, in the exchange's unit order)
//   end
// builds each as SyncRunner::set_units / AsyncRunner::set_inline do (parameter and gradient buffers
// 16-byte aligned, one m and one v per PS) and prints the coalesced pieces per segment, all of
// them coalesced, and the two tail flags.  tests/test_step_audit_cpu.py holds the output against
// the Python twin step_audit.segment_pieces.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../update_plan.h"

using namespace ddl;

static void print(const char* what, const std::vector<PlanPiece>& v) {
  printf("%s", what);
  for (const auto& p : v)
    printf(" %lld %lld %d %lld;", (long long)p.lo, (long long)p.hi, p.ps, (long long)p.state_off);
  printf("\n");
}

int main() {
  constexpr int kMaxPs = 64;
  alignas(16) static float m[kMaxPs][4], v[kMaxPs][4];  // one state base per PS
  alignas(16) static float w[4], g[4];
  char line[256], name[128];
  UpdatePlan plan;
  bool open = false;
  while (fgets(line, sizeof line, stdin)) {
    long long seg, lo, hi, ps, off;
    if (sscanf(line, "plan %127s", name) == 1) {
      plan = UpdatePlan();
      open = true;
    } else if (open && strncmp(line, "end", 3) == 0) {
      plan.finish(reinterpret_cast<uintptr_t>(w), reinterpret_cast<uintptr_t>(g));
      printf("plan %s\n", name);
      for (int s = 0; s < kPlanSegments; ++s) {
        char tag[16];
        snprintf(tag, sizeof tag, "seg %d:", s);
        print(tag, plan.seg[s]);
      }
      print("merged:", plan.merged);
      printf("tail_ok %d tail_v_ok %d\n", (int)plan.tail_ok, (int)plan.tail_v_ok);
      open = false;
    } else if (open && sscanf(line, "%lld %lld %lld %lld %lld", &seg, &lo, &hi, &ps, &off) == 5) {
      if (seg < 0 || seg >= kPlanSegments || ps < 0 || ps >= kMaxPs || lo < 0 || hi < lo) {
        printf("bad piece: %s", line);
        return 1;
      }
      plan.add((int)seg, PlanPiece{lo, hi, off, (int)ps, m[ps], v[ps]});
    } else {
      printf("bad line: %s", line);
      return 1;
    }
  }
  return open ? 1 : 0;
}
