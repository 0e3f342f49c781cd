// K5 — V's preparation, once per call before the sweep (topk.hip's translation unit only):
// the operands' scales, the sweep order (V rows bucketed by decreasing norm), the split f16
// planes of V and the row norms in that order.
#pragma once
#include "topk_split.h"

namespace als {

namespace {

// max |x| over n floats -> *out (ordered uint bits; *out zeroed beforehand).
__global__ __launch_bounds__(256) void tk_absmax_kernel(const float* __restrict__ x, int64_t n,
                                                        unsigned* __restrict__ out) {
  float m = 0.f;
  const int64_t n4 = n >> 2;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  auto fold = [&](const float4& v) {
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {  // four independent loads in flight
    const float4 a = x4[i], b = x4[i + stride], c = x4[i + 2 * stride], d = x4[i + 3 * stride];
    fold(a);
    fold(b);
    fold(c);
    fold(d);
  }
  for (; i < n4; i += stride) fold(x4[i]);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(x[4 * n4 + threadIdx.x]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(out, __float_as_uint(m));  // NaN-free non-negative floats order as uints
  }
}

}  // namespace

// Sweep order: V rows by decreasing norm (4096 log-spaced buckets, 128 per octave;
// order inside a bucket arbitrary).  Large-norm rows carry most top scores, so the
// lists fill with near-final entries early and later rows rarely pass the filter.
// The order only affects speed: insertion compares (score, V row index) exactly.
constexpr int kTkBuckets = 4096;

// 16 lanes per V row: squared norm -> bucket (0 = largest norms).
__device__ __forceinline__ int tk_row_bucket(const float* __restrict__ V, int64_t r, int ld,
                                             int k, float log2_ref) {
  const int l = threadIdx.x & 15;
  float s = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int d = 4 * l + 64 * h;
    if (d < k) {
      const float4 v = *reinterpret_cast<const float4*>(V + r * ld + d);
      s += v.x * v.x + (d + 1 < k ? v.y * v.y : 0.f) + (d + 2 < k ? v.z * v.z : 0.f) +
           (d + 3 < k ? v.w * v.w : 0.f);
    }
  }
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (!(s > 0.f)) return kTkBuckets - 1;
  const float b = (log2_ref - 0.5f * __log2f(s)) * 128.f;  // octaves below the reference
  // (NaN, e.g. an Inf row against an Inf reference: bucket 0)
  return !(b > 0.f) ? 0 : (b >= (float)(kTkBuckets - 1) ? kTkBuckets - 1 : (int)b);
}

__device__ __forceinline__ float tk_log2_ref(const float* __restrict__ scal, int k) {
  // reference norm: max |v| * sqrt(k) bounds every row norm
  return __log2f(fmaxf(scal[1], 1e-30f)) + 0.5f * __log2f((float)k);
}

// Bucket counts: per-workgroup histogram in LDS (rows of similar norm share a
// bucket, so global atomics per row would serialise), flushed once per nonzero bin.
__global__ __launch_bounds__(256) void tk_bucket_hist_kernel(const float* __restrict__ V,
                                                             int64_t n_v, int ld, int k,
                                                             const float* __restrict__ scal,
                                                             int32_t* __restrict__ hist) {
  __shared__ int lh[kTkBuckets];
  for (int b = threadIdx.x; b < kTkBuckets; b += 256) lh[b] = 0;
  __syncthreads();
  const float ref = tk_log2_ref(scal, k);
  for (int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; r < n_v;
       r += ((int64_t)gridDim.x * 256) >> 4) {
    const int b = tk_row_bucket(V, r, ld, k, ref);
    if ((threadIdx.x & 15) == 0) atomicAdd(lh + b, 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kTkBuckets; b += 256)
    if (lh[b]) atomicAdd(hist + b, lh[b]);
}

// Exclusive scan of the bucket counts (one workgroup) -> scatter cursors.
__global__ __launch_bounds__(1024) void tk_bucket_scan_kernel(int32_t* __restrict__ hist) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  int v[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = hist[4 * t + j];
    s += v[j];
  }
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int x = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int run = part[t] - s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    hist[4 * t + j] = run;
    run += v[j];
  }
}

// Scatter with the same grid as the count pass: a workgroup recounts its rows in
// LDS, reserves one range per nonzero bin with one global atomic, then places its
// rows inside those ranges with LDS atomics.
__global__ __launch_bounds__(256) void tk_bucket_scatter_kernel(const float* __restrict__ V,
                                                                int64_t n_v, int ld, int k,
                                                                const float* __restrict__ scal,
                                                                int32_t* __restrict__ cursor,
                                                                int32_t* __restrict__ perm) {
  __shared__ int lh[kTkBuckets];
  for (int b = threadIdx.x; b < kTkBuckets; b += 256) lh[b] = 0;
  __syncthreads();
  const float ref = tk_log2_ref(scal, k);
  const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int64_t rs = ((int64_t)gridDim.x * 256) >> 4;
  for (int64_t r = r0; r < n_v; r += rs) {
    const int b = tk_row_bucket(V, r, ld, k, ref);
    if ((threadIdx.x & 15) == 0) atomicAdd(lh + b, 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kTkBuckets; b += 256)
    if (lh[b]) lh[b] = atomicAdd(cursor + b, lh[b]);  // base of this workgroup's range
  __syncthreads();
  for (int64_t r = r0; r < n_v; r += rs) {
    const int b = tk_row_bucket(V, r, ld, k, ref);
    if ((threadIdx.x & 15) == 0) perm[atomicAdd(lh + b, 1)] = (int32_t)r;
  }
}

// Norms of the scaled V rows in sweep order (16 lanes per table row): the coarse
// filter's error slack and the early-exit bound of topk_split_kernel.
__global__ __launch_bounds__(256) void tk_table_norm_kernel(const float* __restrict__ V,
                                                            int64_t n_v, int ld, int k,
                                                            const float* __restrict__ scal,
                                                            const int32_t* __restrict__ perm,
                                                            float* __restrict__ vnorm) {
  const float sv = ldexpf(1.f, tk_split_exponent(scal[1]));
  const int l = threadIdx.x & 15;
  for (int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4; t < n_v;
       t += ((int64_t)gridDim.x * 256) >> 4) {
    const int64_t r = perm[t];
    float s = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = 4 * l + 64 * h;
      if (d < k) {
        const float4 v = *reinterpret_cast<const float4*>(V + r * ld + d);
        s += v.x * v.x + (d + 1 < k ? v.y * v.y : 0.f) + (d + 2 < k ? v.z * v.z : 0.f) +
             (d + 3 < k ? v.w * v.w : 0.f);
      }
    }
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    // a row with a NaN / Inf entry: an unbounded norm keeps every bound using it open
    if (l == 0) vnorm[t] = s < __builtin_inff() ? sv * sqrtf(s) : __builtin_inff();
  }
}

// V -> split planes in sweep order, table row t = V row perm[t]: hi plane
// [n_v][KQ] = hi(sv v), then lo plane [n_v][KQ] = lo(sv v) (f16), dims >= k zero.
__global__ __launch_bounds__(256) void topk_split_table_kernel(const float* __restrict__ V,
                                                               int64_t n_v, int ld, int k,
                                                               int kq_shift,
                                                               const float* __restrict__ scal,
                                                               const int32_t* __restrict__ perm,
                                                               _Float16* __restrict__ out) {
  const float sv = ldexpf(1.f, tk_split_exponent(scal[1]));
  const int kq = 1 << kq_shift;
  const int64_t total = n_v << kq_shift;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * 256) {
    const int64_t r = e >> kq_shift;
    const int d = (int)(e & (kq - 1));
    const float t = d < k ? sv * V[(int64_t)perm[r] * ld + d] : 0.f;
    _Float16 h, l;
    tk_split(t, h, l);
    out[e] = h;
    out[total + e] = l;
  }
}

}  // namespace als
