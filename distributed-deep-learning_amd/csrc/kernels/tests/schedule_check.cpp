// Host-side run of the launch schedule's decisions (schedule.h), meant for a build with
// -fsanitize=address,undefined: pure C++, no GPU.  Prints the default schedule and, for every
// (op, config, train), `support OP CFG TRAIN HAS EFFECTIVE`; then reads cells from standard input,
// one per line, as differences from the defaults and what is pending:
//   cell cfg OP V | splits OP V | wide OP V | dual V | bfirst MASK | direct V | concurrent V |
//        defer V | pend V | seg S TAIL   (any number, in order; `seg` walks backward segment S with
//        an update tail pending before it or not)
// and prints per cell the choices made and the choice-level branch counts, walking each segment as
// Engine::backward_segment does: the four fused outcomes of segment 3, known only once a launch is
// planned, are one name, seg3_fused; a pending tail counts as tail_consumed where the launch takes
// it and as tail_standalone where it is flushed.  tests/test_dispatch_cells_cpu.py holds the
// output against the Python twin tests/dispatch_cells.py.
#include <cstdio>
#include <sstream>
#include <string>

#include "../schedule.h"

using namespace ddl;

struct Walk {
  int hits[BR_COUNT] = {};
  int fused = 0;
  int pend = 0;
  std::string choices;
  void choice(const char* c) { choices += choices.empty() ? "" : ","; choices += c; }
};

static void walk_pair(const Schedule& s, const OpPair& p, bool& tail, Walk& w) {
  const PairChoice ch = choose_pair(s, p.dgrad, p.wgrad);
  w.choice(ch.kind == PAIR_PACK ? "pack" : ch.kind == PAIR_DUAL ? "dual" : "back_to_back");
  ++w.hits[pair_branch(p.dgrad, ch.kind, ch.defers, w.pend != 0)];
  if (tail) ++w.hits[pair_takes_tail(p.dgrad, ch.kind) ? BR_TAIL_CONSUMED : BR_TAIL_STANDALONE];
  tail = false;
  if (ch.kind == PAIR_PACK && ch.defers) w.pend |= p.dgrad == OP_FC2_DGRAD ? 1 : 2;
  // conv4's dual launch computes the deferred fc weight gradients; after a pair back to back the
  // segment flushes them
  if (p.dgrad == OP_CONV4_DGRAD) w.pend = 0;
}

static void walk_segment(const Schedule& s, int seg, bool tail, Walk& w) {
  if (s.concurrent) {
    w.choice("concurrent");
    ++w.hits[BR_CONCURRENT];
    if (tail) ++w.hits[BR_TAIL_STANDALONE];
    return;
  }
  const Segment& g = kSegment[seg];
  if (g.then >= 0) {
    const Seg3Choice c = choose_seg3(s);
    w.choice(c.fused ? "fused" : "unfused");
    if (c.fused) {
      ++w.fused;
      if (tail) ++w.hits[BR_TAIL_CONSUMED];
      return;
    }
    ++w.hits[BR_SEG3_UNFUSED];
  }
  for (int i = 0; i < g.npairs; ++i) walk_pair(s, g.pair[i], tail, w);
}

static void print_row(const char* what, const int* v) {
  printf("defaults %s", what);
  for (int op = 0; op < OP_COUNT; ++op) printf(" %d", v[op]);
  printf("\n");
}

int main() {
  const Schedule def = Schedule::defaults();
  print_row("cfg", def.cfg);
  print_row("eval_cfg", def.eval_cfg);
  print_row("splits", def.splits);
  print_row("wide", def.wide);
  printf("defaults flags wide_thr=%d dual=%d bfirst=%d concurrent=%d conv1_direct=%d "
         "conv1_wgrad_direct=%d fc_wgrad_defer=%d fc2_in_head=%d eval_kmap2=%d\n",
         def.wide_thr, def.dual, def.dual_bfirst, def.concurrent, def.conv1_direct,
         def.conv1_wgrad_direct, def.fc_wgrad_defer, def.fc2_in_head, def.eval_kmap2);
  printf("configs kwave=%d mf16=%d kw16=%d one_wave", CFG_KWAVE, CFG_MF16, CFG_KW16);
  for (int cfg = 0; cfg <= CFG_KW16; ++cfg)
    if (one_wave_cfg(cfg)) printf(" %d", cfg);
  printf("\n");
  for (int op = 0; op < OP_COUNT; ++op)
    for (int cfg = 0; cfg <= CFG_KW16; ++cfg)
      for (int train = 0; train < 2; ++train)
        printf("support %d %d %d %d %d\n", op, cfg, train, op_has_cfg(op, cfg, train),
               effective_cfg(op, cfg, train));
  char buf[4096];
  int cell = 0;
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string key;
    if (!(in >> key) || key != "cell") continue;
    Schedule s = def;
    Walk w;
    bool bad = false;
    while (in >> key) {
      int a = 0, b = 0;
      const bool per_op = key == "cfg" || key == "splits" || key == "wide" || key == "seg";
      if (!(in >> a) || (per_op && !(in >> b))) { bad = true; break; }
      if (per_op && (a < 0 || a >= (key == "seg" ? kSegments : (int)OP_COUNT))) bad = true;
      if (bad) break;
      if (key == "cfg") s.cfg[a] = b;
      else if (key == "splits") s.splits[a] = b;
      else if (key == "wide") s.wide[a] = b;
      else if (key == "dual") s.dual = a;
      else if (key == "bfirst") s.dual_bfirst = a;
      else if (key == "direct") s.conv1_direct = s.conv1_wgrad_direct = a;
      else if (key == "concurrent") s.concurrent = a;
      else if (key == "defer") s.fc_wgrad_defer = a;
      else if (key == "pend") w.pend = a;
      else if (key == "seg") walk_segment(s, a, b != 0, w);
      else { bad = true; break; }
    }
    if (bad) {
      fprintf(stderr, "cell %d: bad input\n", cell);
      return 2;
    }
    printf("cell %d choices %s hits", cell++, w.choices.c_str());
    for (int b = 0; b < BR_COUNT; ++b)
      if (w.hits[b]) printf(" %s=%d", branch_name(b), w.hits[b]);
    if (w.fused) printf(" seg3_fused=%d", w.fused);
    printf(" pend %d\n", w.pend != 0);
  }
  return 0;
}
