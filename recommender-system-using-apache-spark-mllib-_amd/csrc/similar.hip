// K12 — similar items / similar users: cosine nearest neighbours of a few query vectors
// among the rows of one factor table.
//
// K5 (topk.hip) runs its grid over the QUERY rows and prepares the whole table first; for
// "the neighbours of these 1-16 items among a million" that is one workgroup behind an
// O(n) set-up.  Here the grid runs over the TABLE: the rows are cut into contiguous slices,
// one wavefront (a 64-thread workgroup) per slice, and the raw fp32 table is read once per
// pass of at most 16 queries.
//
// Sweep (sim_sweep_kernel<LPR, C>).  LPR lanes share a table row (16 at rank 33-128, 8 at
// 17-32, 4 below), each holding C float4 of it (coalesced 16-byte loads: a row's lanes read
// consecutive 16 B); a tile is 16 rows per wavefront.  The pass's query vectors sit in LDS,
// dimension-major ([dim][16 queries], each group of four dims skewed by 16 B so the LPR
// distinct addresses of one ds_read_b128 fall on distinct banks; lanes on the same column
// read the same address, a broadcast), so one 16-byte LDS read yields one dimension of four
// queries and feeds every row the lane holds.  Per lane and row: 16 partial dots and the
// partial |t|^2, from the same registers.  The 16 partial dots are reduced across the row's
// lanes as a reduce-scatter (each xor step halves the values a lane carries: 15 shuffles
// for 16 sums at LPR = 16 instead of 64), after which each lane owns the finished dots of
// 16 / LPR queries; |t|^2 takes a plain butterfly.  Both trees pair the same lanes in the
// same order, whatever slot a query has in its pass and whatever slice a row is in, so a
// (query, row) pair's score is the same bits wherever it is computed.
//   score = dot * (1 / sqrt(|t|^2)) * inv|q|        (fp32; inv|q| from an fp64 norm)
// Lists.  Per query a log of `cap` 64-bit keys in LDS (the (monotone score bits | ~index)
// key of rank_key.h, compared exactly).  A key above the query's threshold is appended —
// positions from ballots, no atomics — and a log that the next tile could overflow is cut to
// its `top` largest keys (sim_compact: bitwise search for the top-th key, then a stable
// partition), whose smallest becomes the threshold.  The threshold never exceeds the
// running top-th key, so every key that belongs to the slice's top `top` reaches the log.
// At the end of the slice each query's `top` keys (unordered, padded with 0) go to the
// workspace with plain stores: [query][slice][top].
// Merge (sim_merge_kernel): one wavefront per query streams that query's slice lists
// through the same log, cuts to `top`, ranks the survivors (keys are unique) and unpacks
// idx / score.  More than 64 slices are merged in two stages (groups of 32, then the
// groups).  Nothing depends on the number of slices or on the order workgroups finish.
//
// Unit copy (sim_unit_rows_kernel): t / |t| in fp32 from an fp64 norm, for the many-query
// route that hands the copy to K5; the same launch clears the allow bit of every row that
// cannot be a neighbour (zero norm, NaN, Inf).
#include "als_common.h"
#include "rank_key.h"
#include "sim_lists.h"

#include <algorithm>

namespace als {
namespace {

typedef float sim_f2 __attribute__((ext_vector_type(2)));

// (kSimTopMax, the merge constants, sim_compact, sim_cap, sim_merge_kernel, sim_slices and
// sim_groups: sim_lists.h)
constexpr int kSimPass = 16;       // queries per pass
constexpr int kSimTileRows = 16;   // table rows per tile: the most keys one tile appends per query

// LDS offset (floats) of dimension d's 16 query values: 64 B per dimension, each group of
// four dimensions skewed by a further 16 B.
__device__ __forceinline__ int sim_qoff(int d) { return d * 16 + (d >> 2) * 4; }

template <int LPR, int C>
__global__ __launch_bounds__(64) void sim_sweep_kernel(
    const float* __restrict__ T, int64_t n, int ld, int k, const float* __restrict__ Q, int nq,
    int ldq, const int32_t* __restrict__ self_rows, const uint32_t* __restrict__ allow, int top,
    int64_t rows_per_slice, int slices, uint64_t* __restrict__ out) {
  constexpr int G = 64 / LPR;    // rows per load step
  constexpr int RPT = LPR / 4;   // load steps per tile (G RPT = 16 rows)
  constexpr int VPL = 16 / LPR;  // finished dots per lane and row after the reduce-scatter
  constexpr int KP = 4 * LPR * C;
  constexpr int JC = (sim_cap(kSimTopMax) + 63) / 64;
  static_assert(G * RPT == kSimTileRows, "tile rows");
  extern __shared__ __attribute__((aligned(16))) uint64_t sim_smem[];
  const int cap = sim_cap(top);
  uint64_t* logs = sim_smem;                              // [16][cap]
  uint64_t* thr = logs + kSimPass * cap;                  // [16] thresholds
  float* qs = reinterpret_cast<float*>(thr + kSimPass);   // [KP] dims x 16 queries, skewed
  float* invq = qs + KP * 16 + KP;                        // [16]
  int* cnt = reinterpret_cast<int*>(invq + kSimPass);     // [16] keys in each log
  int* selfr = cnt + kSimPass;                            // [16]

  const int lane = threadIdx.x & 63, sub = lane % LPR, grp = lane / LPR;

  // the pass's queries: vectors to LDS, 1 / |q| from an fp64 norm; a query with zero norm,
  // a NaN or an Inf is dead (threshold nothing exceeds, vector zero)
  for (int j = 0; j < kSimPass; ++j) {
    double ss = 0.0;
    bool fin = true;
    for (int d = lane; d < KP; d += 64) {
      const float x = (j < nq && d < k) ? Q[(int64_t)j * ldq + d] : 0.f;
      fin = fin && (x - x == 0.f);
      ss += (double)x * (double)x;
      qs[sim_qoff(d) + j] = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += shfl_xor_f64(ss, o);
    const float iq = (float)(1.0 / sqrt(ss));
    const bool ok = j < nq && __all(fin) && ss > 0.0 && iq < __builtin_inff();
    if (!ok)
      for (int d = lane; d < KP; d += 64) qs[sim_qoff(d) + j] = 0.f;
    if (lane == 0) {
      invq[j] = ok ? iq : 0.f;
      thr[j] = ok ? 0ull : ~0ull;
      cnt[j] = 0;
      selfr[j] = (ok && self_rows) ? self_rows[j] : -1;
    }
  }
  __syncthreads();
  float iq[VPL];
  int sf[VPL];
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    iq[v] = invq[sub * VPL + v];
    sf[v] = selfr[sub * VPL + v];
  }
  // lanes holding the same queries as this one: every LPR-th lane from `sub`
  uint64_t same = 0;
#pragma unroll
  for (int g = 0; g < G; ++g) same |= 1ull << (LPR * g);
  same <<= sub;
  const uint64_t below = (1ull << lane) - 1;

  const int slice = blockIdx.x;
  const int64_t r0 = std::min<int64_t>(n, slice * rows_per_slice);
  const int64_t r1 = std::min<int64_t>(n, r0 + rows_per_slice);
  for (int64_t base = r0; base < r1; base += kSimTileRows) {
    // a log this tile could overflow is cut to its `top` best first
    uint64_t full = __ballot(lane < kSimPass && cnt[lane & 15] + kSimTileRows > cap);
    while (full) {
      const int j = __builtin_ctzll(full);
      full &= full - 1;
      const uint64_t P = sim_compact<JC>(logs + j * cap, cnt[j], top);
      if (lane == 0) {
        cnt[j] = top;
        thr[j] = P;
      }
      __syncthreads();
    }
    float4 t[RPT][C];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const int64_t row = base + rr * G + grp;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int d0 = 4 * sub + 4 * LPR * c;
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (row < r1 && d0 < k) {  // (d0 < k <= ld and ld % 4 == 0: the 16 bytes are the row's)
          v = *reinterpret_cast<const float4*>(T + row * ld + d0);
          v.y = d0 + 1 < k ? v.y : 0.f;  // columns [k, ld) are never used
          v.z = d0 + 2 < k ? v.z : 0.f;
          v.w = d0 + 3 < k ? v.w : 0.f;
        }
        t[rr][c] = v;
      }
    }
    sim_f2 acc[RPT][8];
    float s[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      s[rr] = 0.f;
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[rr][a] = sim_f2{0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4* qrow =
            reinterpret_cast<const float4*>(qs + sim_qoff(4 * sub + 4 * LPR * c + i));
        const float4 q0 = qrow[0], q1 = qrow[1], q2 = qrow[2], q3 = qrow[3];
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
          const float4 tv = t[rr][c];
          const float x = i == 0 ? tv.x : (i == 1 ? tv.y : (i == 2 ? tv.z : tv.w));
          const sim_f2 xx = sim_f2{x, x};
          acc[rr][0] += xx * sim_f2{q0.x, q0.y};
          acc[rr][1] += xx * sim_f2{q0.z, q0.w};
          acc[rr][2] += xx * sim_f2{q1.x, q1.y};
          acc[rr][3] += xx * sim_f2{q1.z, q1.w};
          acc[rr][4] += xx * sim_f2{q2.x, q2.y};
          acc[rr][5] += xx * sim_f2{q2.z, q2.w};
          acc[rr][6] += xx * sim_f2{q3.x, q3.y};
          acc[rr][7] += xx * sim_f2{q3.z, q3.w};
          s[rr] = fmaf(x, x, s[rr]);
        }
      }
    uint64_t th[VPL];
    int cn[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      th[v] = thr[sub * VPL + v];
      cn[v] = cnt[sub * VPL + v];
    }
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      // reduce-scatter of the 16 dots over the row's LPR lanes; query of val[v] afterwards:
      // sub VPL + v
      float val[16];
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        val[2 * a] = acc[rr][a].x;
        val[2 * a + 1] = acc[rr][a].y;
      }
      float ss = s[rr];
#pragma unroll
      for (int m = LPR / 2, h = 8; m >= 1; m >>= 1, h >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (i < h) {
            const float send = up ? val[i] : val[i + h];
            const float keep = up ? val[i + h] : val[i];
            val[i] = keep + __shfl_xor(send, m);
          }
        ss += __shfl_xor(ss, m);
      }
      const int64_t row = base + rr * G + grp;
      // a neighbour has a finite norm of at least 2^-50 (NaN fails both tests): below that
      // bound |t|^2 and its partial sums lose bits to the subnormal grid (2^-149 a step)
      const bool rowok = row < r1 && ss >= 0x1p-100f && ss < __builtin_inff();
      const float invt = 1.f / sqrtf(ss);
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        const float sc = val[v] * invt * iq[v];
        const uint64_t key = rank_key(sc, (int)row);
        bool pass = rowok && sc == sc && key > th[v];
        if (pass) {  // admissibility only for a key that would be listed
          if ((int)row == sf[v]) pass = false;
          else if (allow && !((allow[row >> 5] >> (row & 31)) & 1u)) pass = false;
        }
        const uint64_t b = __ballot(pass) & same;
        if (pass) logs[(sub * VPL + v) * cap + cn[v] + __popcll(b & below)] = key;
        cn[v] += __popcll(b);
      }
    }
    if (grp == 0) {
#pragma unroll
      for (int v = 0; v < VPL; ++v) cnt[sub * VPL + v] = cn[v];
    }
    __syncthreads();
  }
  // the slice's `top` keys per query (unordered; open slots 0), plain stores
  for (int j = 0; j < kSimPass; ++j) {
    int m = cnt[j];
    if (m > top) {
      sim_compact<JC>(logs + j * cap, m, top);
      m = top;
    }
    uint64_t* o = out + ((int64_t)j * slices + slice) * top;
    for (int e = lane; e < top; e += 64) o[e] = e < m ? logs[j * cap + e] : 0ull;
  }
}

// Unit-norm copy: out row = t / |t| (fp64 norm over columns [0, k), fp32 quotient), columns
// [k, ld) zero; a row with zero norm, a NaN or an Inf becomes zeros, has its bit cleared in
// `allow` (nullable) and 0 in valid_out (nullable).  One wavefront per 32 rows = one mask
// word, 16 lanes per row: each word is read and written by one lane, so no atomics.
__global__ __launch_bounds__(256) void sim_unit_rows_kernel(const float* __restrict__ T, int64_t n,
                                                            int ld, int k, float* __restrict__ out,
                                                            uint32_t* __restrict__ allow,
                                                            int32_t* __restrict__ valid_out) {
  const int lane = threadIdx.x & 63, l = lane & 15;
  const int64_t words = (n + 31) >> 5;
  for (int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6; w < words;
       w += ((int64_t)gridDim.x * 256) >> 6) {
    uint32_t mask = 0;
    for (int step = 0; step < 8; ++step) {
      const int64_t row = 32 * w + 4 * step + (lane >> 4);
      double ss = 0.0;
      int fin = 1;
      if (row < n)
        for (int d0 = 4 * l; d0 < k; d0 += 64) {
          const float4 v = *reinterpret_cast<const float4*>(T + row * ld + d0);
          const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (d0 + i < k) {
              fin &= (x[i] - x[i] == 0.f);
              ss += (double)x[i] * (double)x[i];
            }
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        ss += shfl_xor_f64(ss, o);
        fin &= __shfl_xor(fin, o);
      }
      const bool ok = row < n && fin && ss > 0.0;
      const double inv = ok ? 1.0 / sqrt(ss) : 0.0;
      if (row < n)
        for (int d0 = 4 * l; d0 < ld; d0 += 64) {
          float4 o4 = float4{0.f, 0.f, 0.f, 0.f};
          if (ok && d0 < k) {
            const float4 v = *reinterpret_cast<const float4*>(T + row * ld + d0);
            o4.x = (float)((double)v.x * inv);
            o4.y = d0 + 1 < k ? (float)((double)v.y * inv) : 0.f;
            o4.z = d0 + 2 < k ? (float)((double)v.z * inv) : 0.f;
            o4.w = d0 + 3 < k ? (float)((double)v.w * inv) : 0.f;
          }
          *reinterpret_cast<float4*>(out + row * ld + d0) = o4;
        }
      if (valid_out && l == 0 && row < n) valid_out[row] = ok ? 1 : 0;
      const uint64_t b = __ballot(ok && l == 0);
      const uint32_t nib = (uint32_t)((b & 1) | ((b >> 15) & 2) | ((b >> 30) & 4) | ((b >> 45) & 8));
      mask |= nib << (4 * step);
    }
    if (allow && lane == 0) allow[w] &= mask;
  }
}

}  // namespace
}  // namespace als

using namespace als;

extern "C" {

size_t als_similar_workspace_bytes(int64_t n, int32_t n_q, int32_t top, int32_t slices) {
  (void)n_q;  // the workspace serves one pass of 16 queries at a time
  if (top < 1 || top > kSimTopMax || slices < 0 || slices > kSimMaxSlices || n < 0) return 0;
  const int s = sim_slices(n, top, slices);
  return align_up(sizeof(uint64_t) * kSimPass * (size_t)s * top) +
         align_up(sizeof(uint64_t) * kSimPass * (size_t)sim_groups(s) * top);
}

int als_similar(const float* T, int64_t n, int32_t ld, int32_t k, const float* Q, int64_t n_q,
                int32_t ldq, const int32_t* self_rows, const uint32_t* allow_bits, int32_t top,
                int32_t slices, int32_t* idx_out, float* score_out, void* ws, size_t ws_bytes,
                void* stream) {
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_similar: rank %d not in [1, 128]", k);
  ALS_REQUIRE(top >= 1 && top <= kSimTopMax, ALS_EUNSUPPORTED,
              "als_similar: top %d not in [1, %d]", top, kSimTopMax);
  ALS_REQUIRE(ld >= k && ld % 4 == 0 && ldq >= k && ldq % 4 == 0, ALS_EINVAL,
              "als_similar: bad ld / ldq");
  ALS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) - 1 && n_q >= 0, ALS_EINVAL,
              "als_similar: bad sizes");
  ALS_REQUIRE(slices >= 0 && slices <= kSimMaxSlices, ALS_EINVAL,
              "als_similar: slices %d not in [0, %d]", slices, kSimMaxSlices);
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(Q && idx_out && score_out && (T || n == 0), ALS_EINVAL,
              "als_similar: null pointer");
  ALS_REQUIRE(((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(Q)) & 15) == 0,
              ALS_EINVAL, "als_similar: T and Q must be 16-byte aligned");
  const size_t need = als_similar_workspace_bytes(n, (int32_t)std::min<int64_t>(n_q, kSimPass),
                                                  top, slices);
  ALS_REQUIRE(ws != nullptr && ws_bytes >= need, ALS_EWORKSPACE,
              "als_similar: workspace %zu < %zu", ws_bytes, need);
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_similar: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int s = sim_slices(n, top, slices);
  const int groups = sim_groups(s);
  const int64_t rows_per_slice = std::max<int64_t>(1, (n + s - 1) / s);
  uint64_t* keys = static_cast<uint64_t*>(ws);
  uint64_t* keys2 = reinterpret_cast<uint64_t*>(
      static_cast<char*>(ws) + align_up(sizeof(uint64_t) * kSimPass * (size_t)s * top));
  const int lpr = k <= 16 ? 4 : (k <= 32 ? 8 : 16);
  const int kp = k <= 64 ? 4 * lpr : 128;
  const size_t lds = sizeof(uint64_t) * kSimPass * ((size_t)sim_cap(top) + 1) +
                     sizeof(float) * ((size_t)kp * 17 + kSimPass) + sizeof(int) * 2 * kSimPass;
  for (int64_t q0 = 0; q0 < n_q; q0 += kSimPass) {
    const int nq = (int)std::min<int64_t>(kSimPass, n_q - q0);
    const float* Qp = Q + q0 * ldq;
    const int32_t* sp = self_rows ? self_rows + q0 : nullptr;
#define ALS_SIM_SWEEP(LPR, C)                                                                 \
  sim_sweep_kernel<LPR, C><<<s, 64, lds, st>>>(T, n, ld, k, Qp, nq, ldq, sp, allow_bits, top, \
                                               rows_per_slice, s, keys)
    if (k <= 16) ALS_SIM_SWEEP(4, 1);
    else if (k <= 32) ALS_SIM_SWEEP(8, 1);
    else if (k <= 64) ALS_SIM_SWEEP(16, 1);
    else ALS_SIM_SWEEP(16, 2);
#undef ALS_SIM_SWEEP
    ALS_LAUNCH_CHECK();
    int32_t* io = idx_out + q0 * top;
    float* so = score_out + q0 * top;
    if (groups) {
      sim_merge_kernel<<<dim3(nq, groups), 64, 0, st>>>(keys, s, kSimMergeFan, top, keys2, nullptr,
                                                        nullptr, 0);
      ALS_LAUNCH_CHECK();
      sim_merge_kernel<<<dim3(nq, 1), 64, 0, st>>>(keys2, groups, groups, top, nullptr, io, so, 1);
    } else {
      sim_merge_kernel<<<dim3(nq, 1), 64, 0, st>>>(keys, s, s, top, nullptr, io, so, 1);
    }
    ALS_LAUNCH_CHECK();
  }
  return ALS_OK;
}

int als_similar_unit_rows(const float* T, int64_t n, int32_t ld, int32_t k, float* out,
                          uint32_t* allow_bits, int32_t* valid_out, void* stream) {
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_similar_unit_rows: rank %d not in [1, 128]",
              k);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_similar_unit_rows: bad ld");
  ALS_REQUIRE(n >= 0 && n < (int64_t(1) << 31) - 1, ALS_EINVAL, "als_similar_unit_rows: bad n");
  if (n == 0) return ALS_OK;
  ALS_REQUIRE(T && out, ALS_EINVAL, "als_similar_unit_rows: null pointer");
  ALS_REQUIRE(((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
              ALS_EINVAL, "als_similar_unit_rows: T and out must be 16-byte aligned");
  const int64_t words = (n + 31) >> 5;
  sim_unit_rows_kernel<<<(int)std::min<int64_t>(2048, (words + 3) / 4), 256, 0, as_stream(stream)>>>(
      T, n, ld, k, out, allow_bits, valid_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
