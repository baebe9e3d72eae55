// Accumulate a worker's gradient over K micro-batches on the device (--accum-steps K): the
// gradient buffer g after micro-batch j of K, and the accumulator A (fp32, the buffer's size),
//   j = 0          A[i] := g[i]                  (the bits copied: no memset, no 0 + g)
//   0 < j < K - 1  A[i] := A[i] + g[i]           (one rounded add)
//   j = K - 1      g[i] := (A[i] + g[i]) * r     (one rounded add, then one rounded multiply)
// with r = (float)(1.0 / K) formed on the host in double and rounded once.  After the last
// micro-batch g holds the mean over the K micro-batches (the loss head divides by the batch, so
// this is the mean-loss gradient of K * B images) and everything downstream reads it as it reads
// a single step's gradient.
//
// Only the payload ranges are touched (the table and chunk enumeration of clip_ranges.h): the
// alignment padding of g and of A keeps its bits.  One launch, no host sync, no scratch.  Chunk c
// is handled by one workgroup, whichever the grid gives it; every element is written by exactly
// one lane from values only that lane read, so the bits depend on (contents, ranges, mode, K)
// alone, not on the grid.  A chunk is 16-byte accesses on its aligned body and its ragged first
// and last elements one by one (range bases are not 16-byte aligned in every plan); g and A must
// sit at the same offset from a 16-byte boundary (the launcher checks).  Every load of a chunk
// is issued before the first add.  ops/accum.py is the CPU twin, bit for bit.
#include "api.h"
#include "common.h"

namespace ddl {

constexpr int kAccumVecs = kClipChunk / (4 * kClipThreads);  // 16-B accesses per lane and chunk
static_assert(kClipChunk % (4 * kClipThreads) == 0, "whole passes per full chunk");

template <int MODE>
DDL_DEV float accum_one(float a, float g, float r) {
  if (MODE == kAccumFirst) return g;
  if (MODE == kAccumAdd) return __fadd_rn(a, g);
  return __fmul_rn(__fadd_rn(a, g), r);
}

template <int MODE>
__global__ void __launch_bounds__(kClipThreads)
grad_accum_kernel(ClipRanges t, float* __restrict__ g, float* __restrict__ acc, float r) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < t.nchunks; c += gridDim.x) {
    const ClipChunk ch = clip_chunk(t, c);
    float* gb = g + ch.at;
    float* ab = acc + ch.at;
    const int shift = (int)((reinterpret_cast<uintptr_t>(gb) >> 2) & 3);
    const int head = min((4 - shift) & 3, ch.n);
    const int nv = (ch.n - head) >> 2;  // (at most kClipChunk / 4: kAccumVecs per lane)
    const int tail = ch.n - head - 4 * nv;
    // the ragged ends: lanes 0..2 take the head, lanes 4..6 the tail, one element each
    int e = -1;
    if (tid < head) e = tid;
    else if (tid >= 4 && tid - 4 < tail) e = head + 4 * nv + tid - 4;
    const float4* gp = reinterpret_cast<const float4*>(gb + head);
    const float4* ap = reinterpret_cast<const float4*>(ab + head);
    float ge = 0.f, ae = 0.f;
    float4 gv[kAccumVecs], av[kAccumVecs];
    if (e >= 0) {
      ge = gb[e];
      if (MODE != kAccumFirst) ae = ab[e];
    }
#pragma unroll
    for (int k = 0; k < kAccumVecs; ++k) {
      const int i = tid + kClipThreads * k;
      if (i < nv) {
        gv[k] = gp[i];
        av[k] = MODE != kAccumFirst ? ap[i] : gv[k];  // (the copy reads g only)
      }
    }
    // the mode's destination: A while accumulating, g when finishing
    float* db = MODE == kAccumFinish ? gb : ab;
    float4* dp = reinterpret_cast<float4*>(db + head);
    if (e >= 0) db[e] = accum_one<MODE>(ae, ge, r);
#pragma unroll
    for (int k = 0; k < kAccumVecs; ++k) {
      const int i = tid + kClipThreads * k;
      if (i < nv) {
        float4 o;
        o.x = accum_one<MODE>(av[k].x, gv[k].x, r);
        o.y = accum_one<MODE>(av[k].y, gv[k].y, r);
        o.z = accum_one<MODE>(av[k].z, gv[k].z, r);
        o.w = accum_one<MODE>(av[k].w, gv[k].w, r);
        dp[i] = o;
      }
    }
  }
}

void launch_accum(const ClipRanges& t, float* g, float* acc, int mode, int k, hipStream_t st,
                  int max_grid) {
  if (k < 2) throw std::invalid_argument("launch_accum: K must be at least 2");
  if (mode < kAccumFirst || mode > kAccumFinish)
    throw std::invalid_argument("launch_accum: mode");
  if (!g || !acc || g == acc) throw std::invalid_argument("launch_accum: buffers");
  if (((reinterpret_cast<uintptr_t>(g) ^ reinterpret_cast<uintptr_t>(acc)) & 15) != 0)
    throw std::invalid_argument("launch_accum: g and A differ in 16-byte alignment");
  if (t.nchunks == 0) return;
  const int cap = max_grid > 0 ? max_grid : 2048;
  const dim3 grid(std::min(t.nchunks, cap)), block(kClipThreads);
  const float r = (float)(1.0 / (double)k);
  if (mode == kAccumFirst)
    DDL_LAUNCH(grad_accum_kernel<kAccumFirst>, grid, block, 0, st, t, g, acc, r);
  else if (mode == kAccumAdd)
    DDL_LAUNCH(grad_accum_kernel<kAccumAdd>, grid, block, 0, st, t, g, acc, r);
  else
    DDL_LAUNCH(grad_accum_kernel<kAccumFinish>, grid, block, 0, st, t, g, acc, r);
}

}  // namespace ddl
