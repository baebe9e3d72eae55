// Host-side check of the clip's range table and chunk enumeration (clip_ranges.h), meant for a
// build with -fsanitize=address,undefined: pure C++, no GPU.  For every shape the GPU tests use
// (tests/test_clip_gpu.py) it walks the table as the kernels do and checks that
//   * the chunks tile every range exactly once, in order, each of 1 .. kClipChunk elements;
//   * the sum kernel's index arithmetic — lane t, pass k, component c of a 16-byte load that
//     starts `shift` elements before the chunk — visits every element of the chunk exactly once,
//     never one outside it, and always in slot j % kClipSlots;
//   * the scale kernel's head / vector / tail split covers the chunk exactly once and its vector
//     part starts on a 16-byte boundary;
//   * malformed tables are refused.
// Prints "OK <chunks> chunks" and returns 0, or the first failure and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../clip_ranges.h"

using namespace ddl;

static int fails = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      if (fails++ < 10) {             \
        printf("FAIL %s: ", #c);      \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

static long walk(const std::vector<std::pair<int64_t, int64_t>>& rs, int64_t base_elem) {
  const ClipRanges t = make_clip_ranges(rs);
  long want = 0;
  for (const auto& r : rs) want += (long)((r.second + kClipChunk - 1) / kClipChunk);
  CHECK(t.nchunks == want, "nchunks %d want %ld", t.nchunks, want);
  CHECK(t.n == (int)rs.size(), "n %d", t.n);
  int range = 0;
  int64_t next = t.n ? t.lo[0] : 0;
  std::vector<unsigned char> seen(kClipChunk);
  constexpr int kVecs = kClipChunk / kClipSlots + 1;
  for (int c = 0; c < t.nchunks; ++c) {
    const ClipChunk ch = clip_chunk(t, c);
    while (range < t.n && (t.len[range] == 0 || next == t.lo[range] + t.len[range])) {
      ++range;
      if (range < t.n) next = t.lo[range];
    }
    CHECK(ch.range == range, "chunk %d in range %d, want %d", c, ch.range, range);
    CHECK(ch.at == next, "chunk %d at %lld, want %lld", c, (long long)ch.at, (long long)next);
    CHECK(ch.n >= 1 && ch.n <= kClipChunk, "chunk %d of %d elements", c, ch.n);
    CHECK(ch.at + ch.n <= t.lo[ch.range] + t.len[ch.range], "chunk %d past its range", c);
    next = ch.at + ch.n;
    // the sum kernel's loads (grad_sumsq_kernel), with the buffer at element `base_elem`
    const int shift = (int)((base_elem + ch.at) & 3);
    seen.assign(kClipChunk, 0);
    for (int tid = 0; tid < kClipThreads; ++tid)
      for (int k = 0; k < kVecs; ++k) {
        const int j0 = 4 * tid + kClipSlots * k - shift;
        const bool vec = j0 >= 0 && j0 + 3 < ch.n;
        if (vec) CHECK(((base_elem + ch.at + j0) & 3) == 0, "misaligned 16-B load");
        for (int e = 0; e < 4; ++e) {
          const int j = j0 + e;
          if (j < 0 || j >= ch.n) continue;
          CHECK(((4 * tid + e - shift) & (kClipSlots - 1)) == j % kClipSlots, "slot of %d", j);
          ++seen[j];
        }
      }
    for (int j = 0; j < ch.n; ++j) CHECK(seen[j] == 1, "element %d read %d times", j, seen[j]);
    // the scale kernel's split (grad_scale_dev_kernel)
    const int head = std::min((4 - shift) & 3, ch.n);
    const int nv = (ch.n - head) >> 2;
    const int tail = ch.n - head - 4 * nv;
    CHECK(head >= 0 && head < 4 && tail >= 0 && tail < 4 && head < kClipThreads, "split");
    CHECK(nv == 0 || ((base_elem + ch.at + head) & 3) == 0, "misaligned 16-B store");
    CHECK(head + 4 * nv + tail == ch.n, "split does not cover the chunk");
  }
  while (range < t.n && (t.len[range] == 0 || next == t.lo[range] + t.len[range])) {
    ++range;
    if (range < t.n) next = t.lo[range];
  }
  CHECK(range == t.n, "ranges left over: %d of %d", range, t.n);
  return t.nchunks;
}

template <class F>
static bool refused(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

int main() {
  const int CH = kClipChunk;
  long chunks = 0;
  const int64_t sizes[] = {0, 1, 3, 4, 63, 64, 65, CH - 1, CH, CH + 1, 3 * CH + 5, 257 * CH + 1};
  for (int64_t n : sizes)
    for (int64_t base = 0; base < 4; ++base)
      for (int64_t lo = 0; lo < 2; ++lo) chunks += walk({{lo, n}}, base);
  // the 14 tensors of the model behind 64-element alignment, as the plans lay them out
  const int64_t numel[14] = {800, 32, 51200, 64, 204800, 128, 819200, 256,
                             1048576, 1024, 524288, 512, 5120, 10};
  std::vector<std::pair<int64_t, int64_t>> plan;
  int64_t off = 0;
  for (int64_t n : numel) {
    plan.push_back({off, n});
    off = (off + n + 63) / 64 * 64;
  }
  chunks += walk(plan, 0);
  chunks += walk(plan, 1);
  plan.insert(plan.begin() + 3, {70000, 0});  // an empty range in the middle
  plan.push_back({off, 0});                   // and at the end
  chunks += walk(plan, 0);
  chunks += walk({}, 0);
  // refusals
  std::vector<std::pair<int64_t, int64_t>> many(17, {0, 1});
  CHECK(refused([&] { make_clip_ranges(many); }), "17 ranges accepted");
  CHECK(refused([] { make_clip_ranges({{-1, 4}}); }), "negative lo accepted");
  CHECK(refused([] { make_clip_ranges({{0, -4}}); }), "negative n accepted");
  CHECK(refused([] { make_clip_ranges({{INT64_MAX - 2, 8}}); }), "overflowing range accepted");
  CHECK(refused([] { make_clip_ranges({{8, 8}}, 15); }), "range past the buffer accepted");
  CHECK(refused([] { make_clip_ranges({{0, INT64_MAX / 2}}); }), "2^62 elements accepted");
  CHECK(!refused([] { make_clip_ranges({{8, 8}}, 16); }), "range at the end refused");
  if (fails) {
    printf("%d failures\n", fails);
    return 1;
  }
  printf("OK %ld chunks\n", chunks);
  return 0;
}
