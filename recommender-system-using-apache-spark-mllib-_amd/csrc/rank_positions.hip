// K9 — full-ranking positions and metrics: where every held-out item sits in its row's
// ordering of ALL admissible items (expected percentile rank of Hu, Koren & Volinsky,
// per-row AUC, reciprocal rank).
//
// als_rank_positions sweeps the whole n_q x n_v score matrix (never materialised) and, for
// every relevant entry, counts the admissible other rows that score strictly higher
// (`above`) and equal (`tied`); als_full_rank_metrics reduces the counts to fp64 metrics.
//
// Arithmetic (the version shipped is the fp32 VALU one; the matrix-core form is future
// work).  The score of (q, v) is the fp32 chain
//     s = 0;  for d = 0 .. rank-1:  s = fmaf(q_d, v_d, s)
// in ascending d, one rounding per term.  Every score of the call comes from that one chain
// — the sweep's register tile, the relevant entries' thresholds and the excluded pairs'
// corrections — so a pair scores bit-identically wherever it is computed and a relevant
// item compares equal to itself.  Error bound: the standard one for a recursive fp32 dot
// product of `rank` terms, |s - s*| <= gamma_rank * sum_d |q_d v_d| with gamma_n =
// n u / (1 - n u), u = 2^-24, which is below the contract's tau = 2 * rank * 2^-24 *
// sum_d |q_d v_d| for every rank <= 128 (n u <= 2^-17).  Zero padding terms add nothing:
// fmaf(0, 0, s) = s.  Scores are compared through a monotone 32-bit key of s + 0.f (so
// -0 == +0); NaN scores are never keys.
//
// Layout.  A workgroup of 256 threads owns kRpRows = 32 query rows, kept in LDS transposed
// ([d][row]).  V is swept in tiles of kRpTileV = 128 rows, staged kRpDepth = 32 columns at
// a time ([d][v], row stride 132 words); a thread holds a 4 x 4 register tile (rows
// 4 (t & 7) .., V rows 4 (t >> 3) ..) and reads one float4 of each operand per d.  A V row
// past n_v or outside `allow` is staged as NaN, so its scores are NaN for every query row
// and one s == s test serves the bounds, the allow mask and genuine NaN factors.
//
// Thresholds.  Before a sweep the workgroup fills an LDS table of at most kRpTable = 2048
// relevant entries, shared by its rows (rows take their entries greedily in row order),
// scores them with the chain above, and sorts the table by (row, key) with a bitonic
// network.  An entry that is itself inadmissible (out of range, excluded, not allowed) or
// scores NaN gets the largest key, sorts behind its row's valid entries and is written as
// -1.  Each swept score is placed by an upper-bound binary search among its row's valid
// thresholds (log m, not m) and counted in one of 2 m + 1 bins: "equal to threshold p" or
// "strictly between p and p + 1" (the bin below every threshold is never needed and not
// kept); scores below the row's lowest threshold skip the search.  Exclusions are not
// tested per score: the sweep counts every allowed row, and afterwards the row's excluded
// pairs (duplicates skipped, not-allowed and NaN ones skipped, exactly the rows the sweep
// counted) are scored with the same chain and taken out of their bins and of n_adm.  A
// suffix sum over the bins gives above / tied for every entry; tied subtracts the entry
// itself.  When the rows of a workgroup hold more entries than the table, the workgroup
// sweeps V again for the rest (a single row larger than the table included); n_adm comes
// from the first sweep.  All counts are integers, so the result does not depend on the
// order of the LDS atomics.
#include "als_common.h"
#include "partial_sums.h"
#include "rank_key.h"

namespace als {

constexpr int kRpRows = 32;      // query rows per workgroup
constexpr int kRpTileV = 128;    // V rows per tile
constexpr int kRpDepth = 32;     // columns staged per barrier pair
constexpr int kRpVStride = 132;  // words per staged column (16-byte aligned, off the bank row)
constexpr int kRpTable = 2048;   // relevant entries per pass (power of two, <= 4096: slot bits)
constexpr int kRpThreads = 256;
constexpr uint32_t kRpBadKey = 0xFFFFFFFFu;  // above the key of +inf (0xFF800000)

constexpr int kFrSums = 11;
constexpr int kFrRowsPerBlock = 4;  // one wavefront each
constexpr int kFrMaxBlocks = 4096;

static inline int64_t fr_blocks(int64_t n_q) {
  const int64_t g = (n_q + kFrRowsPerBlock - 1) / kFrRowsPerBlock;
  return g < 1 ? 1 : (g > kFrMaxBlocks ? kFrMaxBlocks : g);
}

// The one score chain of K9 (see the header): ascending d, one fmaf per term.
__device__ __forceinline__ float rp_dot(const float* __restrict__ q, const float* __restrict__ v,
                                        int k) {
  float s = 0.f;
  int d = 0;
  for (; d + 4 <= k; d += 4) {
    const float4 a = *reinterpret_cast<const float4*>(q + d);
    const float4 b = *reinterpret_cast<const float4*>(v + d);
    s = __builtin_fmaf(a.x, b.x, s);
    s = __builtin_fmaf(a.y, b.y, s);
    s = __builtin_fmaf(a.z, b.z, s);
    s = __builtin_fmaf(a.w, b.w, s);
  }
  for (; d < k; ++d) s = __builtin_fmaf(q[d], v[d], s);
  return s;
}

__device__ __forceinline__ uint32_t rp_table_key(const uint64_t* __restrict__ keys, int slot) {
  return (uint32_t)(keys[slot] >> 12);
}

// Count one score (key) of a row whose nv valid thresholds sit at keys[seg .. seg + nv):
// add `delta` to the bin of the last threshold <= key.  Nothing to do below the lowest.
__device__ __forceinline__ void rp_place(const uint64_t* __restrict__ keys, int* __restrict__ cnt,
                                         int seg, int nv, uint32_t key, int delta) {
  int lo = 0, hi = nv;
  while (lo < hi) {  // upper bound
    const int mid = (lo + hi) >> 1;
    if (rp_table_key(keys, seg + mid) <= key) lo = mid + 1;
    else hi = mid;
  }
  if (lo == 0) return;
  const int slot = seg + lo - 1;
  const int eq = rp_table_key(keys, slot) == key ? 1 : 0;
  atomicAdd(&cnt[2 * slot + eq], delta);
}

__global__ __launch_bounds__(kRpThreads) void rank_positions_kernel(
    const float* __restrict__ Q, int64_t n_q, const float* __restrict__ V, int n_v, int ld, int k,
    const int64_t* __restrict__ rel_begin, const int64_t* __restrict__ rel_end,
    const int32_t* __restrict__ rel_col, RowFilter f, int32_t* __restrict__ above,
    int32_t* __restrict__ tied, int32_t* __restrict__ n_adm) {
  extern __shared__ float4 rp_smem[];  // Qs [kp][kRpRows], then Vs [kRpDepth][kRpVStride]
  __shared__ uint64_t keys[kRpTable];  // (row << 44) | (score key << 12) | slot
  __shared__ int cnt[2 * kRpTable];    // [2 slot] between slot and slot + 1, [2 slot + 1] equal
  __shared__ int64_t sBeg[kRpRows];    // next unplaced entry of the row
  __shared__ int sRem[kRpRows], sTake[kRpRows], sSeg[kRpRows], sNv[kRpRows], sAdm[kRpRows];
  __shared__ int sTotal;

  const int t = threadIdx.x;
  const int kp = (k + 3) & ~3;
  float* Qs = reinterpret_cast<float*>(rp_smem);
  float* Vs = Qs + kp * kRpRows;
  const int64_t row0 = (int64_t)blockIdx.x * kRpRows;
  const int nrows = (int)(n_q - row0 < kRpRows ? n_q - row0 : kRpRows);

  for (int idx = t; idx < kp * kRpRows; idx += kRpThreads) {
    const int q = idx / kp, d = idx - q * kp;
    Qs[d * kRpRows + q] = (q < nrows && d < k) ? Q[(row0 + q) * ld + d] : 0.f;
  }
  if (t < kRpRows) {
    int64_t m = 0, b = 0;
    if (t < nrows) {
      b = rel_begin[row0 + t];
      m = rel_end[row0 + t] - b;
      if (m < 0) m = 0;
      if (m > 0x7fffffff) m = 0x7fffffff;
    }
    sBeg[t] = b;
    sRem[t] = (int)m;
    sAdm[t] = 0;
  }
  __syncthreads();

  const int qg = t & 7, vg = t >> 3;
  for (int pass = 0;; ++pass) {
    // ---- rows take their next entries greedily in row order ----
    if (t < 64) {
      const int rem = t < kRpRows ? sRem[t] : 0;
      const int c = rem < kRpTable ? rem : kRpTable;
      int inc = c;  // inclusive scan of the clamped counts (<= 32 * kRpTable: no overflow)
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (t >= o) inc += up;
      }
      const int before = inc - c;
      const int seg = before < kRpTable ? before : kRpTable;
      const int take = rem < kRpTable - seg ? rem : kRpTable - seg;
      if (t < kRpRows) {
        sSeg[t] = seg;
        sTake[t] = take;
        sNv[t] = 0;
      }
      if (t == kRpRows - 1) sTotal = seg + take;
    }
    __syncthreads();
    const int total = sTotal;
    if (pass > 0 && total == 0) break;  // uniform
    int n2 = 2;
    while (n2 < total) n2 <<= 1;

    // ---- the table: one thread per entry scores it and tests its own admissibility ----
    for (int slot = t; slot < n2; slot += kRpThreads) {
      uint64_t kv = ~0ull;
      if (slot < total) {
        int lo = 0, hi = kRpRows;  // the last row with sSeg <= slot
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (sSeg[mid] <= slot) lo = mid;
          else hi = mid;
        }
        const int row = lo;
        const int64_t e = sBeg[row] + (slot - sSeg[row]);
        const int c = rel_col[e];
        uint32_t key = kRpBadKey;
        if (c >= 0 && c < n_v && row_allowed(f, c) && !row_excluded(f, row0 + row, c)) {
          const float s = rp_dot(Q + (row0 + row) * ld, V + (int64_t)c * ld, k);
          if (s == s) key = score_key(s);
        }
        if (key == kRpBadKey) {
          above[e] = -1;
          tied[e] = -1;
        } else {
          atomicAdd(&sNv[row], 1);
        }
        kv = ((uint64_t)row << 44) | ((uint64_t)key << 12) | (uint64_t)slot;
      }
      keys[slot] = kv;
    }
    for (int i = t; i < 2 * kRpTable; i += kRpThreads) cnt[i] = 0;
    __syncthreads();
    for (int k2 = 2; k2 <= n2; k2 <<= 1) {  // bitonic sort of keys[0 .. n2), ascending
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int i = t; i < n2; i += kRpThreads) {
          const int x = i ^ j;
          if (x > i) {
            const uint64_t a = keys[i], b = keys[x];
            if ((a > b) == ((i & k2) == 0)) {
              keys[i] = b;
              keys[x] = a;
            }
          }
        }
        __syncthreads();
      }
    }

    int seg[4], nv[4];
    uint32_t lowkey[4];
    int nloc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      seg[i] = sSeg[4 * qg + i];
      nv[i] = sNv[4 * qg + i];
      lowkey[i] = nv[i] > 0 ? rp_table_key(keys, seg[i]) : kRpBadKey;
    }

    // ---- the sweep ----
    for (int v0 = 0; v0 < n_v; v0 += kRpTileV) {
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
      for (int d0 = 0; d0 < kp; d0 += kRpDepth) {
        const int dn = kp - d0 < kRpDepth ? kp - d0 : kRpDepth;
#pragma unroll
        for (int it = 0; it < kRpTileV * kRpDepth / 4 / kRpThreads; ++it) {
          const int idx = t + kRpThreads * it;
          const int vr = idx >> 3, d = d0 + 4 * (idx & 7);
          const int v = v0 + vr;
          const float nan = __builtin_nanf("");
          float4 x = make_float4(nan, nan, nan, nan);
          if (v < n_v && row_allowed(f, v)) {
            x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (d < kp) {
              x = *reinterpret_cast<const float4*>(V + (int64_t)v * ld + d);
              if (d + 1 >= k) x.y = 0.f;
              if (d + 2 >= k) x.z = 0.f;
              if (d + 3 >= k) x.w = 0.f;
            }
          }
          float* dst = Vs + (4 * (idx & 7)) * kRpVStride + vr;
          dst[0] = x.x;
          dst[kRpVStride] = x.y;
          dst[2 * kRpVStride] = x.z;
          dst[3 * kRpVStride] = x.w;
        }
        __syncthreads();
#pragma unroll 4
        for (int d = 0; d < dn; ++d) {
          const float4 a = *reinterpret_cast<const float4*>(Qs + (d0 + d) * kRpRows + 4 * qg);
          const float4 b = *reinterpret_cast<const float4*>(Vs + d * kRpVStride + 4 * vg);
          const float av[4] = {a.x, a.y, a.z, a.w};
          const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float s = acc[i][j];
          if (s == s) {
            ++nloc[i];
            const uint32_t key = score_key(s);
            if (key >= lowkey[i]) rp_place(keys, cnt, seg[i], nv[i], key, 1);
          }
        }
      }
    }
    if (pass == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) atomicAdd(&sAdm[4 * qg + i], nloc[i]);
    }
    __syncthreads();

    // ---- take the excluded rows the sweep counted back out: one wave per row ----
    if (f.ex_begin) {
      const int lane = t & 63;
      for (int row = t >> 6; row < nrows; row += kRpThreads / 64) {
        const int rnv = sNv[row], rseg = sSeg[row];
        if (pass > 0 && rnv == 0) continue;
        const int64_t beg = f.ex_begin[row0 + row], end = f.ex_end[row0 + row];
        int gone = 0;
        for (int64_t e = beg + lane; e < end; e += 64) {
          const int c = f.ex_col[e];
          if (c < 0 || c >= n_v) continue;
          if (e > beg && f.ex_col[e - 1] == c) continue;  // a duplicate: counted once
          if (!row_allowed(f, c)) continue;                // the sweep never counted it
          const float s = rp_dot(Q + (row0 + row) * ld, V + (int64_t)c * ld, k);
          if (!(s == s)) continue;
          ++gone;
          if (rnv > 0) rp_place(keys, cnt, rseg, rnv, score_key(s), -1);
        }
        if (pass == 0 && gone) atomicAdd(&sAdm[row], -gone);
      }
      __syncthreads();
    }

    // ---- suffix sums: one thread per row walks its thresholds from the top ----
    if (t < nrows) {
      const int rnv = sNv[t], rseg = sSeg[t];
      const int64_t gb = sBeg[t];
      int running = 0, run_above = 0, run_tied = 0;
      for (int p = rnv - 1; p >= 0; --p) {
        const int slot = rseg + p;
        const uint64_t kv = keys[slot];
        const bool run_end = p == rnv - 1 || rp_table_key(keys, slot + 1) != (uint32_t)(kv >> 12);
        if (run_end) {  // only run ends ever receive counts
          const int h = cnt[2 * slot], eq = cnt[2 * slot + 1];
          run_above = running + h;
          run_tied = eq - 1;
          running += h + eq;
        }
        const int64_t e = gb + ((int)(kv & 0xFFF) - rseg);
        above[e] = run_above;
        tied[e] = run_tied;
      }
      if (pass == 0) n_adm[row0 + t] = sAdm[t];
    }
    __syncthreads();
    if (t < kRpRows) {
      sBeg[t] += sTake[t];
      sRem[t] -= sTake[t];
    }
    __syncthreads();
  }
}

// ---- metrics over the counts ----------------------------------------------------------
// One wavefront per query row.  Lane l folds entries l, l + 64, ... of the row in that
// order, the lanes are combined by a fixed xor tree, rows add up per wave in row order,
// the four waves of a block in wave order and the blocks by one final block: bitwise
// reproducible.  sums: 0 sum w pr, 1 sum w, 2 sum of row-mean pr, 3 sum row AUC, 4 AUC rows,
// 5 sum row RR, 6 RR rows, 7 rows with m > 0, 8 valid pairs, 9 dropped pairs, 10 rows with
// a percentile mean (m > 0 and N > 1).
__global__ __launch_bounds__(256) void full_rank_metrics_kernel(
    const int32_t* __restrict__ above, const int32_t* __restrict__ tied,
    const int32_t* __restrict__ n_adm, int64_t n_q, const int64_t* __restrict__ rel_begin,
    const int64_t* __restrict__ rel_end, const float* __restrict__ w,
    double* __restrict__ per_row, double* __restrict__ partial) {
  __shared__ double swave[kFrRowsPerBlock][kFrSums];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double acc[kFrSums];
#pragma unroll
  for (int i = 0; i < kFrSums; ++i) acc[i] = 0.0;
  const double nan = __builtin_nan("");
  const int64_t n_grp = (n_q + kFrRowsPerBlock - 1) / kFrRowsPerBlock;
  for (int64_t g = blockIdx.x; g < n_grp; g += gridDim.x) {
    const int64_t r = g * kFrRowsPerBlock + wv;
    if (r >= n_q) continue;  // wave-uniform
    const int64_t beg = rel_begin[r], end = rel_end[r];
    const double N = (double)n_adm[r];
    double sp = 0.0, swp = 0.0, sw = 0.0, pmin = 1.0e300, m = 0.0, dropped = 0.0;
    for (int64_t e = beg + lane; e < end; e += 64) {
      const int a = above[e];
      if (a < 0) {
        dropped += 1.0;
        continue;
      }
      const double p = (double)a + 0.5 * (double)tied[e];
      const double we = w ? (double)w[e] : 1.0;
      sp += p;
      swp += we * p;
      sw += we;
      pmin = p < pmin ? p : pmin;
      m += 1.0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      sp += shfl_xor_f64(sp, o);
      swp += shfl_xor_f64(swp, o);
      sw += shfl_xor_f64(sw, o);
      m += shfl_xor_f64(m, o);
      dropped += shfl_xor_f64(dropped, o);
      const double other = shfl_xor_f64(pmin, o);
      pmin = other < pmin ? other : pmin;
    }
    double v_pr = nan, v_auc = nan, v_rr = nan;
    acc[9] += dropped;
    if (m > 0.0) {
      acc[7] += 1.0;
      acc[8] += m;
      v_rr = 1.0 / (1.0 + pmin);
      acc[5] += v_rr;
      acc[6] += 1.0;
      if (N > 1.0) {
        acc[0] += swp / (N - 1.0);
        acc[1] += sw;
        v_pr = sp / (N - 1.0) / m;
        acc[2] += v_pr;
        acc[10] += 1.0;
      }
      if (N > m) {
        v_auc = 1.0 - (sp - 0.5 * m * (m - 1.0)) / (m * (N - m));
        acc[3] += v_auc;
        acc[4] += 1.0;
      }
    }
    if (per_row && lane == 0) {
      per_row[r * 3] = v_pr;
      per_row[r * 3 + 1] = v_auc;
      per_row[r * 3 + 2] = v_rr;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kFrSums; ++i) swave[wv][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < kFrSums) {
    double a = 0.0;
    for (int i = 0; i < kFrRowsPerBlock; ++i) a += swave[i][threadIdx.x];
    partial[(int64_t)kFrSums * blockIdx.x + threadIdx.x] = a;
  }
}

}  // namespace als

using namespace als;

extern "C" {

size_t als_full_rank_workspace_bytes(int64_t n_q) {
  return align_up(sizeof(double) * kFrSums * (size_t)fr_blocks(n_q));
}

int32_t als_rank_positions_table(void) { return kRpTable; }

int als_rank_positions(const float* Q, int64_t n_q, const float* V, int64_t n_v, int32_t ld,
                       int32_t k, const int64_t* rel_begin, const int64_t* rel_end,
                       const int32_t* rel_col, const int64_t* ex_begin, const int64_t* ex_end,
                       const int32_t* ex_col, const uint32_t* allow_bits, int32_t* above_out,
                       int32_t* tied_out, int32_t* n_adm_out, void* ws, size_t ws_bytes,
                       void* stream) {
  (void)ws;
  (void)ws_bytes;
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_rank_positions: rank %d outside [1, 128]",
              k);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL,
              "als_rank_positions: ld %d must be a multiple of 4 and >= rank %d", ld, k);
  ALS_REQUIRE(n_q >= 0, ALS_EINVAL, "als_rank_positions: n_q < 0");
  ALS_REQUIRE(n_v >= 0 && n_v < 0x7fffffffLL, ALS_EINVAL,
              "als_rank_positions: n_v outside [0, 2^31 - 1)");
  ALS_REQUIRE(n_q < (int64_t)kRpRows * 0x7fffffffLL, ALS_EINVAL,
              "als_rank_positions: n_q too large");
  const int rc = check_exclusion_args("als_rank_positions", ex_begin, ex_end, ex_col);
  if (rc != ALS_OK) return rc;
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(Q && rel_begin && rel_end && rel_col && above_out && tied_out && n_adm_out,
              ALS_EINVAL, "als_rank_positions: null pointer");
  ALS_REQUIRE(V || n_v == 0, ALS_EINVAL, "als_rank_positions: null V");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(Q) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(V) & 15) == 0,
              ALS_EINVAL, "als_rank_positions: Q and V must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int kp = (k + 3) & ~3;
  const int lds = (int)sizeof(float) * (kp * kRpRows + kRpDepth * kRpVStride);
  ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_positions_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const RowFilter f{ex_begin, ex_end, ex_col, allow_bits};
  const unsigned nb = (unsigned)((n_q + kRpRows - 1) / kRpRows);
  rank_positions_kernel<<<nb, kRpThreads, (size_t)lds, st>>>(
      Q, n_q, V, (int)n_v, ld, k, rel_begin, rel_end, rel_col, f, above_out, tied_out, n_adm_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_full_rank_metrics(const int32_t* above, const int32_t* tied, const int32_t* n_adm,
                          int64_t n_q, const int64_t* rel_begin, const int64_t* rel_end,
                          const float* w, double* sums_out, double* per_row_out, void* ws,
                          size_t ws_bytes, void* stream) {
  ALS_REQUIRE(n_q >= 0, ALS_EINVAL, "als_full_rank_metrics: n_q < 0");
  ALS_REQUIRE(sums_out, ALS_EINVAL, "als_full_rank_metrics: null sums_out");
  hipStream_t st = as_stream(stream);
  if (n_q == 0) {
    ALS_HIP(hipMemsetAsync(sums_out, 0, kFrSums * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(above && tied && n_adm && rel_begin && rel_end, ALS_EINVAL,
              "als_full_rank_metrics: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_full_rank_metrics: workspace not 16-byte aligned");
  ALS_REQUIRE(ws && ws_bytes >= als_full_rank_workspace_bytes(n_q), ALS_EWORKSPACE,
              "als_full_rank_metrics: workspace too small");
  const int64_t nb = fr_blocks(n_q);
  double* partial = static_cast<double*>(ws);
  full_rank_metrics_kernel<<<(unsigned)nb, 256, 0, st>>>(above, tied, n_adm, n_q, rel_begin,
                                                         rel_end, w, per_row_out, partial);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kFrSums><<<1, 256, 0, st>>>(partial, nb, sums_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
