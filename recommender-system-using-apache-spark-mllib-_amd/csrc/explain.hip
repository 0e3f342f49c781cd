// K11 — explain: why was item t recommended to row u?  (als_explain, ABI 9)
//
// A row's factor is the solution of its normal equations, x_u = A_u^-1 b_u with
// b_u = sum_j wb_j y_j over the row's ratings, so every score splits exactly into one term
// per rating:
//   score(u, t) = y_t^T A_u^-1 b_u = sum_j wb_j (z_t . y_j),   z_t = A_u^-1 y_t.
// K7 (fold_in.hip) forms and factors the same A_u but keeps only x_u; this kernel keeps the
// factor in LDS and solves against the targets instead.  The gather / Gram / LDL^T device
// code is shared with K7 through row_system.h, minus b, which is not needed here.
//
// One 256-thread workgroup per row, one launch, no workspace:
//   pass 1   K7's gather + Gram + square-root-free LDL^T: the lower-packed fp64 triangle
//            stays in LDS for the rest of the row.  One factorisation per row, however
//            many targets it has.
//   pass 2   Targets in batches of 16, one 16-lane group per target.  Lane g of a group
//            holds components g, g + 16, ... of y_t in registers; forward and back
//            substitution broadcast one finished component per step with a shuffle inside
//            the group, so the multi-RHS solve needs no barrier and writes LDS once (z_t).
//   pass 3   The row's ratings are streamed again, 32 at a time.  Thread (target, g) forms
//            the dots of entries g and g + 16 with z_t (fp64, columns ascending), then the
//            weight; lane 0 of the group adds the batch's contributions to the score in
//            row order and inserts them into the target's sorted list in LDS.
// Everything a result depends on runs in a fixed order: two calls give the same bits.
#include <algorithm>

#include "row_system.h"

namespace als {

constexpr int kExTargets = 16;       // targets solved per step: one 16-lane group each
constexpr int kExMaxTop = 32;

// Dynamic LDS of one block, byte offsets (all 16-byte multiples).  Unlike K7 the gather
// buffer cannot alias the triangle: pass 3 gathers while the factor is still needed.
// Row strides are padded off the 256-byte bank row: z by 2 doubles, the gather by 4 floats.
struct ExLds {
  int z, sc, lc, diag, inv, wa, wb, ybuf, lp, col, cnt, total;
};

__host__ __device__ static inline ExLds ex_lds(int k, int kp) {
  ExLds l;
  int off = (k * (k + 1) / 2 * 8 + 15) / 16 * 16;          // the packed triangle, k rows
  l.z = off;    off += kExTargets * (kp + 2) * 8;          // z_t per target
  l.sc = off;   off += kExTargets * kRowBatch * 8;          // the batch's contributions
  l.lc = off;   off += kExTargets * kExMaxTop * 8;         // list values, sorted
  l.diag = off; off += kRowMaxRank * 8;                     // diagonal of A as summed
  l.inv = off;  off += kRowMaxRank * 8;                     // 1 / d_j
  l.wa = off;   off += kRowBatch * 8;
  l.wb = off;   off += kRowBatch * 8;
  l.ybuf = off; off += kRowBatch * (kp + 4) * 4;            // gathered factor rows
  l.lp = off;   off += kExTargets * kExMaxTop * 4;         // list entry positions
  l.col = off;  off += kRowBatch * 4;
  l.cnt = off;  off += 16;
  l.total = off;
  return l;
}

__device__ __forceinline__ double ex_shfl16(double v, int src) {  // inside a 16-lane group
  int2 iv = __builtin_bit_cast(int2, v);
  iv.x = __shfl(iv.x, src, 16);
  iv.y = __shfl(iv.y, src, 16);
  return __builtin_bit_cast(double, iv);
}

// NB = k_pad / 16: thread (a, b) owns rows a + 16 p and columns b + 16 q, q <= p < NB.
template <int NB, bool IMPLICIT>
__global__ __launch_bounds__(kRowThreads) void explain_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_rows, const float* __restrict__ Y, int64_t n_src,
    int ld, int k, float reg, float alpha, const double* __restrict__ yty,
    const int64_t* __restrict__ tgt_ptr, const int32_t* __restrict__ tgt, int top_n,
    float* __restrict__ score_out, int32_t* __restrict__ pos_out, float* __restrict__ contrib_out,
    int32_t* __restrict__ n_used_out, int32_t* __restrict__ status) {
  constexpr int KP = 16 * NB;
  constexpr int YS = KP + 4, ZS = KP + 2;
  constexpr int NACC = NB * (NB + 1) / 2;
  extern __shared__ float4 ex_smem[];  // 16-byte aligned
  const ExLds L = ex_lds(k, KP);
  char* const base = reinterpret_cast<char*>(ex_smem);
  double* const Ap = reinterpret_cast<double*>(base);
  double* const sz = reinterpret_cast<double*>(base + L.z);
  double* const sc = reinterpret_cast<double*>(base + L.sc);
  double* const lc = reinterpret_cast<double*>(base + L.lc);
  double* const sdiag = reinterpret_cast<double*>(base + L.diag);
  double* const sinv = reinterpret_cast<double*>(base + L.inv);
  double* const swa = reinterpret_cast<double*>(base + L.wa);
  double* const swb = reinterpret_cast<double*>(base + L.wb);
  float* const ybuf = reinterpret_cast<float*>(base + L.ybuf);
  int* const lp = reinterpret_cast<int*>(base + L.lp);
  int* const scol = reinterpret_cast<int*>(base + L.col);
  int* const scnt = reinterpret_cast<int*>(base + L.cnt);

  const int t = threadIdx.x;
  const int ta = t >> 4, tb = t & 15;  // the Gram's grid; pass 2 / 3: target ta, lane tb
  const int lane = t & 63;

  for (int64_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int64_t pb = row_ptr[row], pe = row_ptr[row + 1];
    const int64_t qb = tgt_ptr[row], qe = tgt_ptr[row + 1];
    const bool work = qe > qb;  // a row without targets is counted, not factored

    // ---- pass 1: gather + Gram (row_system.h)
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    double no_b = 0.0;          // WITH_B = false: b is not summed
    int n_used = 0, n_pos = 0;  // wave 0 only
    for (int64_t s0 = pb; s0 < pe; s0 += kRowBatch) {
      if (t < 64)
        row_weights<IMPLICIT>(s0, pe, col, val, n_src, alpha, lane, scol, swa, swb, n_used, n_pos);
      __syncthreads();
      if (work) {
        row_gather<KP, YS>(Y, ld, k, scol, ybuf, t);
        __syncthreads();
        const int nb = pe - s0 < kRowBatch ? (int)(pe - s0) : kRowBatch;
        row_gram_batch<NB, YS, false>(ybuf, nb, swa, swb, acc, no_b);
      }
      __syncthreads();  // the next batch overwrites scol and ybuf
    }
    if (t == 0) {
      scnt[0] = n_used;
      scnt[1] = n_pos;
    }
    __syncthreads();
    const int n_all = scnt[0];
    const double lam_n = (double)reg * (double)(IMPLICIT ? scnt[1] : n_all);
    if (n_used_out && t == 0) n_used_out[row] = n_all;
    __syncthreads();  // scnt is rewritten by the next row
    if (!work) continue;

    bool ok = n_all > 0;  // no used entry: zero scores and empty lists, not an error
    if (ok) {
#pragma unroll
      for (int p = 0; p < NB; ++p) {
#pragma unroll
        for (int q = 0; q <= p; ++q) {
          const int i = ta + 16 * p, j = tb + 16 * q;
          if (i < k && j <= i) {
            const int e = i * (i + 1) / 2 + j;
            double a = acc[p * (p + 1) / 2 + q];
            if (IMPLICIT) a += yty[e];
            if (i == j) {
              a += lam_n;
              sdiag[i] = a;  // the diagonal of A as summed: the scale of pivot i's rounding error
            }
            Ap[e] = a;
          }
        }
      }
      __syncthreads();
      ok = row_ldlt<false>(Ap, sdiag, k);
      if (!ok && t == 0) atomicCAS(status, 0, (int32_t)(row + 1));
    }
    if (!ok) {  // uniform: the row's slots read as "nothing to explain"
      const int64_t n_out = (qe - qb) * top_n;
      for (int64_t i = t; i < n_out; i += kRowThreads) {
        pos_out[qb * top_n + i] = -1;
        contrib_out[qb * top_n + i] = 0.f;
      }
      for (int64_t i = qb + t; i < qe; i += kRowThreads) score_out[i] = 0.f;
      __syncthreads();
      continue;
    }
    if (t < k) sinv[t] = 1.0 / Ap[t * (t + 1) / 2 + t];
    __syncthreads();
    double sv[NB];  // 1 / d_i of this lane's components
#pragma unroll
    for (int p = 0; p < NB; ++p) sv[p] = tb + 16 * p < k ? sinv[tb + 16 * p] : 0.0;

    for (int64_t q0 = qb; q0 < qe; q0 += kExTargets) {
      // ---- pass 2: z = A^-1 y_t, target q0 + ta, components tb + 16 p in registers
      const int64_t slot = q0 + ta;
      const bool live = slot < qe;
      int tid = -1;
      if (live) tid = tgt[slot];
      const bool known = tid >= 0 && (int64_t)tid < n_src;
      double w[NB];
#pragma unroll
      for (int p = 0; p < NB; ++p) {
        const int i = tb + 16 * p;
        w[p] = known && i < k ? (double)Y[(int64_t)tid * ld + i] : 0.0;
      }
      // forward: w <- L^-1 y, column by column; component j lives in lane j % 16
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        for (int jl = 0; jl < 16; ++jl) {
          const int j = 16 * jb + jl;
          if (j >= k) break;
          const double cj = ex_shfl16(w[jb], jl) * sinv[j];
#pragma unroll
          for (int p = jb; p < NB; ++p) {
            const int i = tb + 16 * p;
            if (i > j && i < k) w[p] = fma(-Ap[i * (i + 1) / 2 + j], cj, w[p]);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < NB; ++p) w[p] *= sv[p];  // D^-1
      // back: L^T z = w from the last component up
#pragma unroll
      for (int lb = NB - 1; lb >= 0; --lb) {
        for (int ll = 15; ll >= 0; --ll) {
          const int l = 16 * lb + ll;
          if (l >= k) continue;
          const double zl = ex_shfl16(w[lb], ll);
#pragma unroll
          for (int p = 0; p <= lb; ++p) {
            const int i = tb + 16 * p;
            if (i < l) w[p] = fma(-(Ap[l * (l + 1) / 2 + i] * sv[p]), zl, w[p]);
          }
        }
      }
#pragma unroll
      for (int p = 0; p < NB; ++p) sz[ta * ZS + tb + 16 * p] = w[p];  // zeros from k on
      __syncthreads();

      // ---- pass 3: contributions, score and the sorted list
      double score = 0.0;  // lane 0 of the group
      int n_list = 0;
      const int k4 = (k + 3) & ~3;
      for (int64_t s0 = pb; s0 < pe; s0 += kRowBatch) {
        if (t < 64) {
          int u0 = 0, u1 = 0;
          row_weights<IMPLICIT>(s0, pe, col, val, n_src, alpha, lane, scol, swa, swb, u0, u1);
        }
        __syncthreads();
        row_gather<KP, YS>(Y, ld, k, scol, ybuf, t);
        __syncthreads();
        if (known) {
          const double* zt = sz + ta * ZS;
          const float* y0 = ybuf + tb * YS;
          const float* y1 = ybuf + (tb + 16) * YS;
          double d0 = 0.0, d1 = 0.0;
          for (int c = 0; c < k4; c += 4) {  // columns [k, k4) are zeros on both sides
            const float4 a = *reinterpret_cast<const float4*>(y0 + c);
            const float4 b = *reinterpret_cast<const float4*>(y1 + c);
            const double z0 = zt[c], z1 = zt[c + 1], z2 = zt[c + 2], z3 = zt[c + 3];
            d0 = fma(z0, (double)a.x, d0);
            d1 = fma(z0, (double)b.x, d1);
            d0 = fma(z1, (double)a.y, d0);
            d1 = fma(z1, (double)b.y, d1);
            d0 = fma(z2, (double)a.z, d0);
            d1 = fma(z2, (double)b.z, d1);
            d0 = fma(z3, (double)a.w, d0);
            d1 = fma(z3, (double)b.w, d1);
          }
          // the dot first, then the weight: equal items with equal ratings tie bit for bit;
          // + 0.0 turns the -0 of a zero weight into +0
          sc[ta * kRowBatch + tb] = swb[tb] * d0 + 0.0;
          sc[ta * kRowBatch + tb + 16] = swb[tb + 16] * d1 + 0.0;
        }
        __syncthreads();
        if (known && tb == 0) {
          const int nb = pe - s0 < kRowBatch ? (int)(pe - s0) : kRowBatch;
          double* const vc = lc + ta * kExMaxTop;
          int* const vp = lp + ta * kExMaxTop;
          for (int e = 0; e < nb; ++e) {
            if (scol[e] < 0) continue;  // not a used entry: no candidate
            const double c = sc[ta * kRowBatch + e];
            score += c;                 // every contribution, in row order
            // entries come in ascending position: an equal value goes behind
            if (n_list == top_n && !(c > vc[top_n - 1])) continue;
            int i = n_list < top_n ? n_list : top_n - 1;
            while (i > 0 && vc[i - 1] < c) {
              vc[i] = vc[i - 1];
              vp[i] = vp[i - 1];
              --i;
            }
            vc[i] = c;
            vp[i] = (int)(s0 - pb) + e;
            if (n_list < top_n) ++n_list;
          }
        }
        __syncthreads();  // the next batch overwrites scol, ybuf and sc
      }
      n_list = __shfl(n_list, 0, 16);
      if (live) {
        if (tb == 0) score_out[slot] = (float)score;
        for (int i = tb; i < top_n; i += 16) {
          const bool f = i < n_list;
          pos_out[slot * top_n + i] = f ? lp[ta * kExMaxTop + i] : -1;
          contrib_out[slot * top_n + i] = f ? (float)lc[ta * kExMaxTop + i] : 0.f;
        }
      }
      __syncthreads();  // sz and the lists are rewritten by the next targets
    }
  }
}

}  // namespace als

using namespace als;

extern "C" {

size_t als_explain_workspace_bytes(int64_t n_rows, int32_t k) {
  (void)n_rows;
  (void)k;
  return 0;  // every intermediate lives in registers and LDS
}

int als_explain(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                const float* Y_src, int64_t n_src, int32_t ld, int32_t k, float reg, int implicit,
                float alpha, const double* yty_packed, const int64_t* tgt_ptr, const int32_t* tgt,
                int32_t top_n, float* score, int32_t* contrib_pos, float* contrib,
                int32_t* n_used_out, int32_t* status_dev, void* ws, size_t ws_bytes,
                void* stream) {
  (void)ws;
  (void)ws_bytes;
  if (int rc = row_check_args("als_explain", k, ld, n_rows, n_src, reg, alpha, implicit,
                              yty_packed))
    return rc;
  ALS_REQUIRE(top_n >= 1 && top_n <= kExMaxTop, ALS_EUNSUPPORTED,
              "als_explain: top_n %d not in [1, %d]", top_n, kExMaxTop);
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(row_ptr && col && val && tgt_ptr && tgt && score && contrib_pos && contrib &&
                  status_dev,
              ALS_EINVAL, "als_explain: null pointer");
  if (int rc = row_check_source("als_explain", n_src, Y_src, nullptr)) return rc;
  hipStream_t st = as_stream(stream);
  const int nb = als_k_pad(k) / 16;
  const int lds = ex_lds(k, 16 * nb).total;
  const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kRowMaxBlocks);
  return row_dispatch(nb, implicit, [&](auto nbc, auto imp) -> int {
    constexpr auto kernel = &explain_kernel<decltype(nbc)::value, decltype(imp)::value>;
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    kernel<<<grid, kRowThreads, lds, st>>>(row_ptr, col, val, n_rows, Y_src, n_src, ld, k, reg,
                                           alpha, yty_packed, tgt_ptr, tgt, top_n, score,
                                           contrib_pos, contrib, n_used_out, status_dev);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  });
}

}  // extern "C"
