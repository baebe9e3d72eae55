// Clip a worker's gradient by its global norm (tf.clip_by_global_norm on the worker, ahead of
// apply_gradients): norm = sqrt(sum of g^2 over the payload ranges), coef = C / norm when
// norm > C, else exactly 1; the gradient is scaled in place.  Two launches, no host sync: the
// coefficient stays on the device ({norm, coef} in a two-float buffer).
//
// The result is a pure function of (contents, ranges, C): every addition has a fixed place.
//   * chunk c (clip_ranges.h: kClipChunk elements, enumerated range by range) is summed by one
//     workgroup, whichever one the grid gives it;
//   * element j of the chunk is widened to double and its square (exact in double) added to
//     slot j % 1024, in increasing j, each slot starting from +0;
//   * the 1024 slots fold to 256 as (s[i] + s[i+256]) + (s[i+512] + s[i+768]), the 256 to one by
//     halving, s[i] += s[i+h] for h = 128 .. 1 (through LDS);
//   * the last workgroup to arrive (conv1.h c1w_arrive: write-through partials + an arrival
//     ticket, re-zeroed by the last arriver) adds partial[i], i = t, t + 256, ... in increasing i
//     into lane t's sum and folds the 256 sums by the same halving;
//   * sqrt and C / norm are formed in double and rounded once to float.
// Slots belong to element indices, not addresses: a chunk that starts `shift` elements past a
// 16-byte boundary is read with the same aligned 16-byte loads, lane t's four components then
// holding slots (4t + c - shift) mod 1024, and the chunk's ragged first and last vectors read
// element by element.  Only fp64 summation rounds: |norm - exact| <= 1 ulp of float.
// ops/clip.py is the CPU twin of this order, bit for bit.
#include "api.h"
#include "common.h"
#include "conv1.h"

namespace ddl {

constexpr int kClipVecs = kClipChunk / kClipSlots + 1;  // 16-B loads per lane and chunk (+1: shift)
static_assert(kClipSlots == 4 * kClipThreads, "one float4 per lane and pass");
static_assert(kClipChunk % kClipSlots == 0, "whole passes per full chunk");

// the 256 per-lane sums in s[0..255] -> their sum in every lane (halving, fixed order)
DDL_DEV double clip_fold256(double* s, int tid) {
#pragma unroll
  for (int h = kClipThreads / 2; h >= 1; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
  return s[0];
}

DDL_DEV void clip_store_partial(brsrc_t pr, int c, double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  __builtin_amdgcn_raw_buffer_store_b32((unsigned)b, pr, c * 8, 0, 16);
  __builtin_amdgcn_raw_buffer_store_b32((unsigned)(b >> 32), pr, c * 8 + 4, 0, 16);
}
DDL_DEV double clip_load_partial(brsrc_t pr, int c) {
  const uint64_t lo = __builtin_amdgcn_raw_buffer_load_b32(pr, c * 8, 0, 16);
  const uint64_t hi = __builtin_amdgcn_raw_buffer_load_b32(pr, c * 8 + 4, 0, 16);
  return __builtin_bit_cast(double, lo | (hi << 32));
}

__global__ void __launch_bounds__(kClipThreads)
grad_sumsq_kernel(ClipRanges t, const float* __restrict__ g, float max_norm,
                  float* __restrict__ out2, double* __restrict__ partial,
                  int* __restrict__ ticket) {
  __shared__ double sl[kClipSlots];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const brsrc_t pr = make_rsrc(partial, (uint32_t)t.nchunks * 8u);
  for (int c = blockIdx.x; c < t.nchunks; c += gridDim.x) {
    const ClipChunk ch = clip_chunk(t, c);
    const float* base = g + ch.at;
    const int shift = (int)((reinterpret_cast<uintptr_t>(base) >> 2) & 3);
    // every load of the chunk is issued before any is summed
    float4 v[kClipVecs];
#pragma unroll
    for (int k = 0; k < kClipVecs; ++k) {
      const int j0 = 4 * tid + kClipSlots * k - shift;  // (base + j0 is 16-B aligned)
      if (j0 >= 0 && j0 + 3 < ch.n) {
        v[k] = ld4(base + j0);
      } else {
        v[k].x = (j0 >= 0 && j0 < ch.n) ? base[j0] : 0.f;
        v[k].y = (j0 + 1 >= 0 && j0 + 1 < ch.n) ? base[j0 + 1] : 0.f;
        v[k].z = (j0 + 2 >= 0 && j0 + 2 < ch.n) ? base[j0 + 2] : 0.f;
        v[k].w = (j0 + 3 >= 0 && j0 + 3 < ch.n) ? base[j0 + 3] : 0.f;
      }
    }
    // (an absent element adds +0 to a sum that is never negative: no bit changes)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int k = 0; k < kClipVecs; ++k) {
      const double x = v[k].x, y = v[k].y, z = v[k].z, w = v[k].w;
      a0 += x * x;  // (exact products: fused or not, the same bits)
      a1 += y * y;
      a2 += z * z;
      a3 += w * w;
    }
    __syncthreads();  // the previous chunk's fold has read sl[0]
    sl[(4 * tid + 0 - shift) & (kClipSlots - 1)] = a0;
    sl[(4 * tid + 1 - shift) & (kClipSlots - 1)] = a1;
    sl[(4 * tid + 2 - shift) & (kClipSlots - 1)] = a2;
    sl[(4 * tid + 3 - shift) & (kClipSlots - 1)] = a3;
    __syncthreads();
    const double s = (sl[tid] + sl[tid + 256]) + (sl[tid + 512] + sl[tid + 768]);
    __syncthreads();
    sl[tid] = s;
    __syncthreads();
    const double sum = clip_fold256(sl, tid);
    if (tid == 0) clip_store_partial(pr, c, sum);
  }
  if (!c1w_arrive(ticket, (int)gridDim.x, &flag)) return;
  double s = 0.0;
  for (int i = tid; i < t.nchunks; i += kClipThreads) s += clip_load_partial(pr, i);
  sl[tid] = s;
  __syncthreads();
  const double total = clip_fold256(sl, tid);
  if (tid == 0) {
    const double nd = __dsqrt_rn(total);
    const float norm = (float)nd;
    float coef = 1.f;
    // not finite (an inf / nan element, or a norm past float's range): the gradient is left
    // as it is and the norm reported
    if (isfinite(norm) && nd > (double)max_norm) coef = (float)__ddiv_rn((double)max_norm, nd);
    out2[0] = norm;
    out2[1] = coef;
  }
}

// g[i] *= *coef over the same chunks: 16-byte accesses, the chunk's ragged ends element by
// element.  coef == 1: the whole grid returns (wave-uniform), no element is rewritten.
__global__ void __launch_bounds__(kClipThreads)
grad_scale_dev_kernel(ClipRanges t, float* __restrict__ g, const float* __restrict__ out2) {
  const float a = out2[1];
  if (a == 1.f) return;
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < t.nchunks; c += gridDim.x) {
    const ClipChunk ch = clip_chunk(t, c);
    float* base = g + ch.at;
    const int shift = (int)((reinterpret_cast<uintptr_t>(base) >> 2) & 3);
    const int head = min((4 - shift) & 3, ch.n);
    const int nv = (ch.n - head) >> 2;
    const int tail = ch.n - head - 4 * nv;
    if (tid < head) base[tid] *= a;
    float4* p = reinterpret_cast<float4*>(base + head);
    for (int i = tid; i < nv; i += kClipThreads) {
      float4 x = p[i];
      x.x *= a;
      x.y *= a;
      x.z *= a;
      x.w *= a;
      p[i] = x;
    }
    if (tid < tail) base[head + 4 * nv + tid] *= a;
  }
}

void launch_clip(const ClipRanges& t, float* g, float max_norm, float* out2, double* partials,
                 int* ticket, hipStream_t st, int max_grid) {
  if (!(max_norm > 0.f)) throw std::invalid_argument("launch_clip: max_norm must be positive");
  const int cap = max_grid > 0 ? max_grid : 1024;
  const int grid = std::max(1, std::min(t.nchunks, cap));
  DDL_LAUNCH(grad_sumsq_kernel, dim3(grid), dim3(kClipThreads), 0, st, t, g, max_norm, out2,
             partials, ticket);
  DDL_LAUNCH(grad_scale_dev_kernel, dim3(grid), dim3(kClipThreads), 0, st, t, g, out2);
}

}  // namespace ddl
