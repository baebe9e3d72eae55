// Range table and chunk enumeration of the global-norm clip (clip.hip).  Pure C++ (no HIP): the
// host-side sanitizer program csrc/kernels/tests/clip_ranges_check.cpp builds it alone.
//
// The payload of the gradient buffer is a table of at most kClipMaxRanges element ranges
// [lo, lo + n) in plan order.  Work is cut into chunks of kClipChunk elements, enumerated range by
// range; a range's last chunk may be short, an empty range has no chunk.  Chunk c's sum of
// squares goes to partial[c], so the number of partials is a function of the table alone.
#pragma once
#include <stdint.h>

#include <stdexcept>
#include <utility>
#include <vector>

namespace ddl {

constexpr int kClipMaxRanges = 16;
constexpr int kClipChunk = 8192;   // elements per chunk (CH)
constexpr int kClipSlots = 1024;   // element j of a chunk accumulates in slot j % kClipSlots
constexpr int kClipThreads = 256;

struct ClipRanges {
  int n = 0;                         // ranges in use
  int nchunks = 0;                   // chunks of all ranges
  int64_t lo[kClipMaxRanges] = {};   // first element of range r in the gradient buffer
  int64_t len[kClipMaxRanges] = {};  // its element count
  int first[kClipMaxRanges + 1] = {};  // first chunk of range r (first[n] = nchunks)
};

// the table of `(lo, n)` ranges, in the order given; `total` > 0: every range must lie inside
// [0, total)
inline ClipRanges make_clip_ranges(const std::vector<std::pair<int64_t, int64_t>>& lo_n,
                                   int64_t total = 0) {
  if (lo_n.size() > (size_t)kClipMaxRanges)
    throw std::invalid_argument("clip: more than 16 ranges");
  ClipRanges t;
  int64_t chunks = 0;
  for (const auto& r : lo_n) {
    if (r.first < 0 || r.second < 0) throw std::invalid_argument("clip: negative range");
    if (r.first > INT64_MAX - r.second) throw std::invalid_argument("clip: range overflows");
    if (total > 0 && r.first + r.second > total)
      throw std::invalid_argument("clip: range past the end of the buffer");
    t.lo[t.n] = r.first;
    t.len[t.n] = r.second;
    t.first[t.n] = (int)chunks;
    // (n / CH + (n % CH != 0): no n + CH - 1, which could overflow)
    chunks += r.second / kClipChunk + (r.second % kClipChunk != 0);
    if (chunks > (int64_t)1 << 24) throw std::invalid_argument("clip: too many chunks");
    ++t.n;
  }
  for (int r = t.n; r <= kClipMaxRanges; ++r) t.first[r] = (int)chunks;
  t.nchunks = (int)chunks;
  return t;
}

// chunk c of table t: its range, first element in the buffer and element count
struct ClipChunk {
  int range;
  int64_t at;
  int n;
};
#if defined(__HIPCC__)
__host__ __device__
#endif
inline ClipChunk clip_chunk(const ClipRanges& t, int c) {
  int r = 0;
  while (r + 1 < t.n && c >= t.first[r + 1]) ++r;
  const int64_t off = (int64_t)(c - t.first[r]) * kClipChunk;
  const int64_t left = t.len[r] - off;
  return ClipChunk{r, t.lo[r] + off, (int)(left < kClipChunk ? left : kClipChunk)};
}

}  // namespace ddl
