// The index rule of shuffled, shift-augmented batches on the device — bit-identical to
// ops/shuffle.py (perm, shift_of).  perm(i; N, key) is a bijection on [0, N): a balanced Feistel
// network of kBatchRounds rounds over 2 * hbits bits (the smallest even width that holds N - 1, at
// least 2), cycle-walked until the value is < N.  A Feistel network permutes its whole domain
// whatever the round function, so the walk from an i < N stays on that permutation's cycle
// through i and comes back below N: callers guarantee i < N (launch_assemble_batch checks).
#pragma once
#include "common.h"

namespace ddl {

constexpr int kBatchRounds = 4;
constexpr uint32_t kBatchGolden = 0x9E3779B9u;
constexpr int kBatchImage = 28;
constexpr int kBatchRow = kBatchImage * kBatchImage;  // floats per image
constexpr int kBatchRowVecs = kBatchRow / 4;          // 16-byte pieces per image (7 per line)
constexpr int kBatchMaxShift = 8;

// the scalars of one batch (ops/shuffle.py: batch_key, half_bits)
struct BatchRule {
  uint32_t n;          // training rows
  uint32_t base;       // position of the batch's row 0 before permutation (slot * B)
  uint32_t key;        // the permutation's key
  uint32_t key_shift;  // the shift's key
  int hbits;           // bits of one Feistel half
  int s;               // shifts in [-s, s]; 0: none
  int shuffle;
};

DDL_DEV uint32_t batch_perm(uint32_t i, const BatchRule& r) {
  const uint32_t mask = (1u << r.hbits) - 1u;
  uint32_t k[kBatchRounds];
#pragma unroll
  for (int j = 0; j < kBatchRounds; ++j) k[j] = ddl_mix32(r.key + (uint32_t)j * kBatchGolden);
  uint32_t x = i;
  do {
    uint32_t left = x >> r.hbits, right = x & mask;
#pragma unroll
    for (int j = 0; j < kBatchRounds; ++j) {
      const uint32_t t = left ^ (ddl_mix32(right ^ k[j]) & mask);
      left = right;
      right = t;
    }
    x = (left << r.hbits) | right;
  } while (x >= r.n);
  return x;
}

// (dx, dy) of the draw at position i, each in [-s, s] (s > 0)
DDL_DEV void batch_shift(uint32_t i, const BatchRule& r, int* dx, int* dy) {
  const uint32_t h = ddl_mix32(i ^ r.key_shift);
  const uint32_t m = 2u * (uint32_t)r.s + 1u;
  *dx = (int)((h & 0xFFFFu) % m) - r.s;
  *dy = (int)((h >> 16) % m) - r.s;
}

}  // namespace ddl
