// Fused optimizer updates on a flat parameter shard (one launch per shard range).
//
// TF1 ApplyAdam (mnist_sync/parameter_server.py:21,26-27), written in
// TF's own update form [TF-semantics]:
//   m += (g - m) * (1 - beta1);  v += (g*g - v) * (1 - beta2);
//   w -= lr_t * m / (sqrt(v) + eps),  lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
// lr_t is computed on the host per PS step counter.  `scale` folds a 1/W gradient mean
// (or 1.0 for the reference's sum) into the same pass.  HBM-bound: 5 streams of fp32;
// 16-byte vector path (+ scalar tail) when every operand is 16-B aligned.
// Momentum SGD (mu = 0: plain SGD, m left holding the scaled gradient): 3 streams read and 2
// written.  The rule itself is update.h's; the two kernel shapes below are instantiated per kind,
// so each instance streams only what its rule has.
#include "common.h"
#include "api.h"

namespace ddl {

// 16-B body over n4 = n / 4 float4 elements; the n % 4 tail element(s) by the first lanes.
// m (copy rule) and v (every rule but Adam) may be null: they are not touched.
template <int KIND>
__global__ void __launch_bounds__(256)
update_vec_kernel(float4* __restrict__ w, const float4* __restrict__ g, float4* __restrict__ m,
                  float4* __restrict__ v, int64_t n, UpdRule r, float step) {
  const int64_t n4 = n >> 2;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = gid; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 W = w[i];
    upd4_state<KIND>(r, step, W, g[i], m, v, i);
    w[i] = W;
  }
  if (gid < (n & 3)) {
    const int64_t e = 4 * n4 + gid;
    upd1_at<KIND>(r, step, reinterpret_cast<float*>(w), reinterpret_cast<const float*>(g)[e],
                  reinterpret_cast<float*>(m), reinterpret_cast<float*>(v), e);
  }
}
// the same update one element per lane (any alignment): upd1 pins the roundings, so both shapes
// give the same bits
template <int KIND>
__global__ void __launch_bounds__(256)
update_scalar_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                     float* __restrict__ v, int64_t n, UpdRule r, float step) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    upd1_at<KIND>(r, step, w, g[i], m, v, i);
}

__global__ void __launch_bounds__(256) scale_kernel(float* __restrict__ p, int64_t n, float a) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] *= a;
}
static int grid_for(int64_t n, int max_grid = 2048) {
  int64_t b = (n + 255) / 256;
  if (b > max_grid) b = max_grid;  // (2048: 8 blocks per CU) grid-stride beyond
  return b < 1 ? 1 : (int)b;
}

template <int KIND>
static void launch_update_kind(const UpdRule& r, float step, const UpdSpan& s, const float* g,
                               int64_t n, hipStream_t st, int max_grid) {
  // only the streams the rule has decide the shape
  const uintptr_t al = (uintptr_t)s.w | (uintptr_t)g | (KIND != kUpdCopy ? (uintptr_t)s.m : 0) |
                       (KIND == kUpdAdam ? (uintptr_t)s.v : 0);
  if ((al & 15) == 0) {
    DDL_LAUNCH(update_vec_kernel<KIND>, dim3(grid_for((n + 3) / 4, max_grid)), dim3(256), 0, st,
               (float4*)s.w, (const float4*)g, (float4*)s.m, (float4*)s.v, n, r, step);
  } else {
    DDL_LAUNCH(update_scalar_kernel<KIND>, dim3(grid_for(n, max_grid)), dim3(256), 0, st, s.w, g,
               s.m, s.v, n, r, step);
  }
}

void launch_update(const UpdRule& r, float step, const UpdSpan& s, const float* g, int64_t n,
                   hipStream_t st, int max_grid) {
  if (n <= 0) return;
  switch (r.kind) {
    case kUpdAdam: launch_update_kind<kUpdAdam>(r, step, s, g, n, st, max_grid); break;
    case kUpdMomentum: launch_update_kind<kUpdMomentum>(r, step, s, g, n, st, max_grid); break;
    case kUpdCopy: launch_update_kind<kUpdCopy>(r, step, s, g, n, st, max_grid); break;
    default: throw std::invalid_argument("launch_update: unknown rule kind");
  }
}

void launch_scale(float* p, int64_t n, float a, hipStream_t st) {
  if (n <= 0) return;
  DDL_LAUNCH(scale_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, n, a);
}
}  // namespace ddl
