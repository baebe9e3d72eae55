// Assemble one training batch on the device (--shuffle, --augment-shift S): xb[B,784] and yb[B]
// from the resident training set and the scalars of batch.h BatchRule.  Row n of the batch is
// training row perm(base + n) (base + n unshuffled), translated by the draw's (dx, dy):
//   xb[n][r][c] = x_train[row][r - dy][c - dx] inside the 28 x 28 image, else 0.0f.
// One launch on the step's stream, no index array read or written, no host sync, no scratch.
//
// One wave per image: the source row, dx and dy depend on the block index alone, so they are
// wave-uniform (the cycle walk runs once per image).  An image is 196 16-byte pieces, 7 per line
// of 28 pixels, so a piece never crosses a line; a lane takes pieces lane, lane + 64, ... and
// issues every load of its pieces before its first store.  Without a shift (SHIFT = false) a
// piece is one 16-byte load: rows are 3136 B and both bases 16-byte aligned (the launcher
// checks).  With one, the source of a piece sits dy * 28 + dx elements off: four element loads,
// each at its bounds-tested offset (an element outside the image becomes 0.0f), adjacent lanes
// reading adjacent addresses; the stores stay 16 bytes wide.  Rows from B on of xb and yb are not touched.  ops/shuffle.py assemble_batch is the CPU
// twin: pure data movement, equal bits.
#include "api.h"
#include "batch.h"

namespace ddl {

constexpr int kBatchThreads = 64;
constexpr int kBatchVecs = (kBatchRowVecs + kBatchThreads - 1) / kBatchThreads;  // per lane
static_assert(kBatchImage % 4 == 0, "a 16-byte piece stays inside one line");

template <bool SHIFT>
__global__ void __launch_bounds__(kBatchThreads)
assemble_batch_kernel(BatchRule r, const float* __restrict__ x_train,
                      const int64_t* __restrict__ y_train, float* __restrict__ xb,
                      int64_t* __restrict__ yb) {
  const uint32_t n = blockIdx.x;  // (the grid is exactly B blocks)
  const uint32_t pos = r.base + n;
  const uint32_t row = r.shuffle ? batch_perm(pos, r) : pos;
  const float* src = x_train + (size_t)row * kBatchRow;
  f32x4* dst = reinterpret_cast<f32x4*>(xb + (size_t)n * kBatchRow);
  const int tid = threadIdx.x;
  int dx = 0, dy = 0;
  if (SHIFT) batch_shift(pos, r, &dx, &dy);
  // Loads are unconditional, so they all issue back to back: a lane past the image's last piece
  // re-reads that piece, and an element outside the shifted image reads the image's element 0;
  // neither value is used.
  f32x4 v[kBatchVecs];
#pragma unroll
  for (int k = 0; k < kBatchVecs; ++k) {
    const int i = min(tid + kBatchThreads * k, kBatchRowVecs - 1);
    if (!SHIFT) {
      v[k] = reinterpret_cast<const f32x4*>(src)[i];
    } else {
      const int sr = i / (kBatchImage / 4) - dy;        // source line
      const int sc = 4 * (i % (kBatchImage / 4)) - dx;  // source column of the piece's element 0
      const bool line = sr >= 0 && sr < kBatchImage;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = line && sc + j >= 0 && sc + j < kBatchImage;
        const float e = src[in ? sr * kBatchImage + sc + j : 0];
        v[k][j] = in ? e : 0.0f;
      }
    }
  }
  const int64_t label = y_train[row];
#pragma unroll
  for (int k = 0; k < kBatchVecs; ++k) {
    const int i = tid + kBatchThreads * k;
    if (i < kBatchRowVecs) dst[i] = v[k];
  }
  if (tid == 0) yb[n] = label;
}

void launch_assemble_batch(const float* x_train, const int64_t* y_train, int64_t n, float* xb,
                           int64_t* yb, int B, int64_t base, uint32_t key, uint32_t key_shift,
                           int s, bool shuffle, hipStream_t st) {
  if (!x_train || !y_train || !xb || !yb) throw std::invalid_argument("assemble_batch: buffers");
  if (n < 1 || n > INT32_MAX) throw std::invalid_argument("assemble_batch: rows in 1..2^31 - 1");
  if (B < 1 || base < 0 || base + (int64_t)B > n)
    throw std::invalid_argument("assemble_batch: the batch lies outside the training rows");
  if (s < 0 || s > kBatchMaxShift) throw std::invalid_argument("assemble_batch: shift in 0..8");
  if (((reinterpret_cast<uintptr_t>(x_train) | reinterpret_cast<uintptr_t>(xb)) & 15) != 0)
    throw std::invalid_argument("assemble_batch: x_train and xb must be 16-byte aligned");
  BatchRule r;
  r.n = (uint32_t)n;
  r.base = (uint32_t)base;
  r.key = key;
  r.key_shift = key_shift;
  int bits = 0;  // bitlength(n - 1)
  while (bits < 32 && ((uint64_t)(n - 1) >> bits) != 0) ++bits;
  r.hbits = (std::max(2, bits) + 1) / 2;
  r.s = s;
  r.shuffle = shuffle ? 1 : 0;
  const dim3 grid(B), block(kBatchThreads);
  if (s > 0)
    DDL_LAUNCH(assemble_batch_kernel<true>, grid, block, 0, st, r, x_train, y_train, xb, yb);
  else
    DDL_LAUNCH(assemble_batch_kernel<false>, grid, block, 0, st, r, x_train, y_train, xb, yb);
}

}  // namespace ddl
