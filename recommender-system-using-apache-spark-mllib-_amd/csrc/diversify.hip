// K14 — diversified lists: maximal marginal relevance (MMR) re-ranking of a candidate pool
// and the intra-list similarity (ILS) of any lists.
//
// One query row per wavefront (a 64-thread workgroup), in the style of K7 / K11 / K13: the
// row's small problem — a pool of m <= 256 candidates of rank k <= 128 — lives in LDS and
// registers from the gather to the last pick.
//
// Gather (div_gather<C>).  16 lanes share a candidate's factor row, each with C float4 of it
// (coalesced 16-byte loads; C = 1 up to rank 64, 2 above), four candidates per
// wave-instruction and sixteen in flight before the first is used.  Per candidate: the norm
// in fp64 over columns [0, k) (columns [k, ld) are masked, whatever they hold), a finite
// flag, and the unit vector (float)(v / |v|) into LDS; a dead slot, a zero norm or a
// non-finite entry gives a zero row, whose cosine with everything is 0.  Only live slots are
// fetched, and an index is range-checked before it is used as an address.
// LDS image: [m][stride] fp32 with stride = 4 (ceil(k / 4) | 1) floats — four times an odd
// number, so the sixteen lanes of one ds_read_b128 group, each on its own candidate row at
// the same column, start 16 B x odd apart and cover the 64 banks once.  68 floats at rank
// 64, 132 at rank 128: with the 1 KiB pick list 18 KiB for a pool of 64 at rank 64 (eight rows
// per CU), 133 KiB for 256 at rank 128 (one).
//
// Greedy loop (div_mmr_kernel<J, C>, J = pool bucket / 64).  Candidate j sits in lane j % 64,
// register j / 64, with its relevance (fp64), the running maximum (fp32) and the running sum
// (fp64) of its cosines to the picked set.  A step: every lane forms value = lam rel -
// (1 - lam) max for its unpicked live candidates (step 0: rel alone, no penalty term, so
// lam = 1 never multiplies an infinity by zero); a butterfly argmax on the pair (value, slot)
// — larger value, then lower slot — leaves the pick in every lane; the picked candidate's
// running sum joins the list's pair sum; its unit row is read from LDS as a broadcast while
// each lane reads its own J rows, one fp32 dot per candidate in a fixed column order; max and
// sum are updated.  top x m dots per row, never m^2 / 2.  No atomics: two calls give the same
// bits.
//
// ILS of given lists (div_ils_kernel<J, C>): the same gather, then for s = 0 .. m - 1 the
// broadcast of row s against every later live slot, summed in fp64 per lane and reduced in a
// fixed butterfly.
#include "als_common.h"

#include <algorithm>
#include <type_traits>

namespace als {
namespace {

constexpr int kDivMaxPool = 256;
constexpr int kDivMaxRank = 128;

// LDS row stride in floats: four times an odd number, >= k rounded up to 4.
__host__ __device__ constexpr int div_stride(int k) { return 4 * (((k + 3) / 4) | 1); }

__device__ __forceinline__ bool div_finite(float x) { return x - x == 0.f; }

// Unit vectors of the row's m slots into rows[slot * stride + d], d < 4 ceil(k / 4).  sc
// (nullable): a slot whose score is not finite is dead.  All 64 lanes must call.
template <int C>
__device__ __forceinline__ void div_gather(const float* __restrict__ V, int64_t n_v, int ld, int k,
                                           const int32_t* __restrict__ ids,
                                           const float* __restrict__ sc, int m, int stride,
                                           float* __restrict__ rows) {
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int kp = (k + 3) & ~3;
  for (int base = 0; base < m; base += 16) {
    float4 v[4][C];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int slot = base + 4 * u + g;
      int32_t id = -1;
      if (slot < m) {
        id = ids[slot];
        if (sc && !div_finite(sc[slot])) id = -1;
      }
      const bool live = id >= 0 && (int64_t)id < n_v;
#pragma unroll
      for (int h = 0; h < C; ++h) {
        const int d0 = 4 * c + 64 * h;
        float4 x = float4{0.f, 0.f, 0.f, 0.f};
        if (live && d0 < k) {  // (d0 < k <= ld and ld % 4 == 0: the 16 bytes are the row's)
          x = *reinterpret_cast<const float4*>(V + (int64_t)id * ld + d0);
          x.y = d0 + 1 < k ? x.y : 0.f;  // columns [k, ld) are never used
          x.z = d0 + 2 < k ? x.z : 0.f;
          x.w = d0 + 3 < k ? x.w : 0.f;
        }
        v[u][h] = x;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int slot = base + 4 * u + g;
      double ss = 0.0;
      int fin = 1;
#pragma unroll
      for (int h = 0; h < C; ++h) {
        const float x[4] = {v[u][h].x, v[u][h].y, v[u][h].z, v[u][h].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fin &= div_finite(x[i]) ? 1 : 0;
          ss += (double)x[i] * (double)x[i];
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        ss += shfl_xor_f64(ss, o);
        fin &= __shfl_xor(fin, o);
      }
      const bool ok = fin && ss > 0.0;
      const double inv = ok ? 1.0 / sqrt(ss) : 0.0;
#pragma unroll
      for (int h = 0; h < C; ++h) {
        const int d0 = 4 * c + 64 * h;
        if (slot < m && d0 < kp) {
          float4 o4 = float4{0.f, 0.f, 0.f, 0.f};
          if (ok) {
            o4.x = (float)((double)v[u][h].x * inv);
            o4.y = (float)((double)v[u][h].y * inv);
            o4.z = (float)((double)v[u][h].z * inv);
            o4.w = (float)((double)v[u][h].w * inv);
          }
          *reinterpret_cast<float4*>(rows + slot * stride + d0) = o4;
        }
      }
    }
  }
}

// acc[jj] = <row s, this lane's row jj> in fp32, columns in ascending order.  s is uniform.
template <int J>
__device__ __forceinline__ void div_dots(const float* __restrict__ rows, int stride, int nc4, int s,
                                         const int (&own)[J], float (&acc)[J]) {
  const float4* __restrict__ pr = reinterpret_cast<const float4*>(rows + s * stride);
#pragma unroll
  for (int jj = 0; jj < J; ++jj) acc[jj] = 0.f;
  for (int c4 = 0; c4 < nc4; ++c4) {
    const float4 p = pr[c4];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      const float4 o = reinterpret_cast<const float4*>(rows + own[jj])[c4];
      acc[jj] = fmaf(p.x, o.x, acc[jj]);
      acc[jj] = fmaf(p.y, o.y, acc[jj]);
      acc[jj] = fmaf(p.z, o.z, acc[jj]);
      acc[jj] = fmaf(p.w, o.w, acc[jj]);
    }
  }
}

template <int J, int C>
__global__ __launch_bounds__(64) void div_mmr_kernel(
    const float* __restrict__ V, int64_t n_v, int ld, int k, const int32_t* __restrict__ idx,
    const float* __restrict__ score, int m, int top, double lam, int32_t* __restrict__ out_idx,
    float* __restrict__ out_score, double* __restrict__ out_ils) {
  extern __shared__ __attribute__((aligned(16))) float div_smem[];
  const int stride = div_stride(k), nc4 = (k + 3) >> 2;
  float* rows = div_smem;                                  // [m][stride]
  int* picks = reinterpret_cast<int*>(rows + m * stride);  // [kDivMaxPool] slots, pick order
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x;
  const int32_t* ids = idx + row * m;
  const float* sc = score + row * m;

  div_gather<C>(V, n_v, ld, k, ids, sc, m, stride, rows);

  float s[J];
  bool avail[J];
  int own[J];
  float smin = __builtin_inff(), smax = -__builtin_inff();
  int n_live = 0;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int slot = 64 * jj + lane;
    s[jj] = 0.f;
    avail[jj] = false;
    if (slot < m) {
      const int32_t id = ids[slot];
      s[jj] = sc[slot];
      avail[jj] = id >= 0 && (int64_t)id < n_v && div_finite(s[jj]);
    }
    if (avail[jj]) {
      smin = fminf(smin, s[jj]);
      smax = fmaxf(smax, s[jj]);
    }
    n_live += __popcll(__ballot(avail[jj]));
    own[jj] = std::min(slot, m - 1) * stride;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    smin = fminf(smin, __shfl_xor(smin, o));
    smax = fmaxf(smax, __shfl_xor(smax, o));
  }
  double rel[J], sum[J];
  float mx[J];
  const double span = (double)smax - (double)smin;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    rel[jj] = smax == smin ? 1.0 : ((double)s[jj] - (double)smin) / span;
    sum[jj] = 0.0;
    mx[jj] = -__builtin_inff();
  }
  __syncthreads();  // the unit rows are in LDS

  const int want = std::min(top, n_live);
  const double pen = 1.0 - lam;
  double pair_sum = 0.0;
  for (int t = 0; t < want; ++t) {
    double bv = -__builtin_inf();
    int bs = 0x7fffffff;
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {  // slots ascend with jj: a strict > keeps the lowest
      const double val = t == 0 ? rel[jj] : lam * rel[jj] - pen * (double)mx[jj];
      if (avail[jj] && val > bv) {
        bv = val;
        bs = 64 * jj + lane;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = shfl_xor_f64(bv, o);
      const int os = __shfl_xor(bs, o);
      if (ov > bv || (ov == bv && os < bs)) {
        bv = ov;
        bs = os;
      }
    }
    bs = __builtin_amdgcn_readfirstlane(bs);  // (every lane holds it; want <= n_live: a slot)
    const int pl = bs & 63, pj = bs >> 6;
    double ps = 0.0;
#pragma unroll
    for (int jj = 0; jj < J; ++jj)
      if (jj == pj) {
        ps = sum[jj];
        if (lane == pl) avail[jj] = false;
      }
    pair_sum += readlane_f64(ps, pl);
    if (lane == 0) picks[t] = bs;
    float acc[J];
    div_dots<J>(rows, stride, nc4, bs, own, acc);
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
      mx[jj] = fmaxf(mx[jj], acc[jj]);
      sum[jj] += (double)acc[jj];
    }
  }
  __syncthreads();  // picks
  for (int e = lane; e < top; e += 64) {
    int32_t oi = -1;
    float os = -__builtin_inff();
    if (e < want) {
      const int sl = picks[e];
      oi = ids[sl];
      os = sc[sl];
    }
    out_idx[row * top + e] = oi;
    out_score[row * top + e] = os;
  }
  if (lane == 0)
    out_ils[row] = want >= 2 ? pair_sum / (0.5 * (double)want * (double)(want - 1))
                             : __builtin_nan("");
}

template <int J, int C>
__global__ __launch_bounds__(64) void div_ils_kernel(const float* __restrict__ V, int64_t n_v,
                                                     int ld, int k,
                                                     const int32_t* __restrict__ idx, int m,
                                                     double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float div_smem[];
  const int stride = div_stride(k), nc4 = (k + 3) >> 2;
  float* rows = div_smem;
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x;
  const int32_t* ids = idx + row * m;

  div_gather<C>(V, n_v, ld, k, ids, nullptr, m, stride, rows);

  bool live[J];
  uint64_t mask[J];
  int own[J];
  int n_live = 0;
#pragma unroll
  for (int jj = 0; jj < J; ++jj) {
    const int slot = 64 * jj + lane;
    live[jj] = false;
    if (slot < m) {
      const int32_t id = ids[slot];
      live[jj] = id >= 0 && (int64_t)id < n_v;
    }
    mask[jj] = __ballot(live[jj]);
    n_live += __popcll(mask[jj]);
    own[jj] = std::min(slot, m - 1) * stride;
  }
  __syncthreads();
  double sum = 0.0;
  for (int s = 0; s < m; ++s) {
    uint64_t ms = 0;
#pragma unroll
    for (int jj = 0; jj < J; ++jj)
      if (jj == (s >> 6)) ms = mask[jj];
    if (!((ms >> (s & 63)) & 1ull)) continue;  // (uniform)
    float acc[J];
    div_dots<J>(rows, stride, nc4, s, own, acc);
#pragma unroll
    for (int jj = 0; jj < J; ++jj)
      if (live[jj] && 64 * jj + lane > s) sum += (double)acc[jj];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += shfl_xor_f64(sum, o);
  if (lane == 0)
    out[row] = n_live >= 2 ? sum / (0.5 * (double)n_live * (double)(n_live - 1))
                           : __builtin_nan("");
}

size_t div_rows_bytes(int m, int k) { return sizeof(float) * (size_t)m * div_stride(k); }

// f(J tag, C tag) for the pool bucket (64 / 128 / 256 slots) and rank class of a call.
template <class F>
int div_dispatch(int m, int k, F&& f) {
  const int j = (m + 63) / 64;
  auto c1 = std::integral_constant<int, 1>{};
  auto c2 = std::integral_constant<int, 2>{};
  auto c4 = std::integral_constant<int, 4>{};
  if (k <= 64) return j <= 1 ? f(c1, c1) : (j <= 2 ? f(c2, c1) : f(c4, c1));
  return j <= 1 ? f(c1, c2) : (j <= 2 ? f(c2, c2) : f(c4, c2));
}

int div_check_table(const char* who, int64_t n_v, int32_t ld, int32_t k,
                    int64_t n_q, int32_t m) {
  ALS_REQUIRE(k >= 1 && k <= kDivMaxRank, ALS_EUNSUPPORTED, "%s: rank %d not in [1, %d]", who, k,
              kDivMaxRank);
  ALS_REQUIRE(m >= 1 && m <= kDivMaxPool, ALS_EUNSUPPORTED, "%s: pool %d not in [1, %d]", who, m,
              kDivMaxPool);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "%s: bad ld", who);
  ALS_REQUIRE(n_v >= 0 && n_v < (int64_t(1) << 31) && n_q >= 0 && n_q < (int64_t(1) << 31) - 1,
              ALS_EINVAL, "%s: bad sizes", who);
  return ALS_OK;
}

}  // namespace
}  // namespace als

using namespace als;

extern "C" {

int als_diversify(const float* V, int64_t n_v, int32_t ld, int32_t k, const int32_t* idx,
                  const float* score, int64_t n_q, int32_t m, int32_t top, float lam,
                  int32_t* out_idx, float* out_score, double* out_ils, void* stream) {
  const int rc = div_check_table("als_diversify", n_v, ld, k, n_q, m);
  if (rc != ALS_OK) return rc;
  ALS_REQUIRE(top >= 1 && top <= m, ALS_EINVAL, "als_diversify: top %d not in [1, pool %d]", top,
              m);
  ALS_REQUIRE(lam >= 0.f && lam <= 1.f, ALS_EINVAL, "als_diversify: lam %g not in [0, 1]",
              (double)lam);  // (a NaN fails both comparisons)
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(idx && score && out_idx && out_score && out_ils && (V || n_v == 0), ALS_EINVAL,
              "als_diversify: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(V) & 15) == 0, ALS_EINVAL,
              "als_diversify: V must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int lds = (int)(div_rows_bytes(m, k) + sizeof(int) * kDivMaxPool);
  return div_dispatch(m, k, [&](auto jc, auto cc) -> int {
    constexpr auto kernel = &div_mmr_kernel<decltype(jc)::value, decltype(cc)::value>;
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    kernel<<<(unsigned)n_q, 64, (size_t)lds, st>>>(V, n_v, ld, k, idx, score, m, top, (double)lam,
                                                   out_idx, out_score, out_ils);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  });
}

int als_list_similarity(const float* V, int64_t n_v, int32_t ld, int32_t k, const int32_t* idx,
                        int64_t n_q, int32_t m, double* out, void* stream) {
  const int rc = div_check_table("als_list_similarity", n_v, ld, k, n_q, m);
  if (rc != ALS_OK) return rc;
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(idx && out && (V || n_v == 0), ALS_EINVAL, "als_list_similarity: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(V) & 15) == 0, ALS_EINVAL,
              "als_list_similarity: V must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int lds = (int)div_rows_bytes(m, k);
  return div_dispatch(m, k, [&](auto jc, auto cc) -> int {
    constexpr auto kernel = &div_ils_kernel<decltype(jc)::value, decltype(cc)::value>;
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    kernel<<<(unsigned)n_q, 64, (size_t)lds, st>>>(V, n_v, ld, k, idx, m, out);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  });
}

}  // extern "C"
