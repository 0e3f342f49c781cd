// K10 — the training objective: the function whose row-wise minimiser als_solve_half computes.
//
// Spark's ALS has no counterpart (ml/recommendation/ALS.scala never evaluates its loss); the
// semantics are those of its NormalEquation / CholeskySolver, lambda scaled by numExplicits:
//   explicit  L = sum_obs (r - s)^2 + lambda (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)
//   implicit  L = sum_all c (p - s)^2 + lambda (sum_u n+_u |x_u|^2 + sum_i n+_i |y_i|^2)
// with s = x_u . y_i, c = 1 + alpha |r|, p = [r > 0] (unobserved pairs c = 1, p = 0), n the
// ratings of a row and n+ those with r > 0.  The all-pairs sum is never formed:
//   sum_all c (p - s)^2 = <X^T X, Y^T Y>_F + sum_obs [c (p - s)^2 - s^2].
//
// Three device pieces, all fp64 over the stored fp32 factors, no atomics, fixed order:
//   objective_side_kernel   one CSR side split by RATINGS: a block owns kObjSpan consecutive
//       ratings and each of its 16 sixteen-lane groups kObjGroupSpan of them.  A group finds
//       its first row by binary search in row_ptr and walks rows forward, keeping its row of X
//       (as doubles) and |x|^2 in registers while the row does not change; it loads 16 (col,
//       val) at a time, gathers the Y rows four ratings ahead and forms s as K4's pair_dot
//       does.  The weighted regulariser sum_row n_row |x_row|^2 is fused: it is sum over the
//       group's runs of (weighted ratings of the run) * |x_row|^2, one product per run, so a
//       row cut by a span boundary adds n1 |x|^2 + n2 |x|^2.  Y = NULL skips the gathers
//       (regulariser and counts only).
//   gram_f64_kernel         F^T F of an n x ld fp32 table in fp64 on the matrix cores
//       (v_mfma_f64_16x16x4_f64): a block owns a run of rows, wave w the 16-row bands w and
//       w + 4 of the 16 x 16 output tiles; a lane converts one float per tile column band and
//       four table rows go into each instruction, A and B operands from the same registers, no
//       LDS.  Columns >= k and rows past the end enter as 0.
//   fold kernels            per-block partials are summed in ascending block order (each
//       thread a strided ascending subsequence, then a fixed tree for the scalar sums:
//       partial_sums.h).
#include "als_common.h"
#include "partial_sums.h"

namespace als {

constexpr int kObjGroupSpan = 64;                   // ratings per 16-lane group
constexpr int kObjSpan = 16 * kObjGroupSpan;        // ratings per block (als_objective_span)
constexpr int kObjOut = 5;                          // data, |data|, reg, n, n_positive
constexpr int kGramMaxBlocks = 256;
constexpr int kGramMinRows = 64;                    // rows per block at least (a multiple of 4)

typedef double double4_t __attribute__((ext_vector_type(4)));

// The calling group's slice of row `row` of X as doubles (columns 4 g .. 4 g + 3 and the same
// + 64; 0 at and past k) and |x|^2 over the whole row, returned to every lane.
__device__ __forceinline__ double load_x_row(const float* __restrict__ X, int64_t row, int ld,
                                             int k, int g, double (&x)[8]) {
  double xx = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int d0 = 4 * g + 64 * h;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d0 < k) a = *reinterpret_cast<const float4*>(X + row * ld + d0);
    x[4 * h + 0] = (double)a.x;
    x[4 * h + 1] = d0 + 1 < k ? (double)a.y : 0.0;
    x[4 * h + 2] = d0 + 2 < k ? (double)a.z : 0.0;
    x[4 * h + 3] = d0 + 3 < k ? (double)a.w : 0.0;
    if (d0 >= k) x[4 * h + 0] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) xx += x[4 * h + j] * x[4 * h + j];
  }
#pragma unroll
  for (int msk = 8; msk >= 1; msk >>= 1) xx += shfl_xor_f64(xx, msk);
  return xx;
}

__global__ __launch_bounds__(256) void objective_side_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t nnz, int32_t n_rows, int32_t n_cols,
    const float* __restrict__ X, const float* __restrict__ Y, int ld, int k, int implicit,
    double alpha, double* __restrict__ partial) {
  __shared__ double sm[kObjOut * 16];
  const int grp = threadIdx.x >> 4, g = threadIdx.x & 15;
  int64_t e = (int64_t)blockIdx.x * kObjSpan + (int64_t)grp * kObjGroupSpan;
  const int64_t e_end = e + kObjGroupSpan < nnz ? e + kObjGroupSpan : nnz;
  // every lane of a group carries the same sums; lane 0 stores them
  double data = 0.0, sabs = 0.0, reg = 0.0, cnt = 0.0, pos = 0.0;
  if (e < e_end) {  // uniform across the group
    // first row: row_ptr[lo] <= e < row_ptr[lo + 1] (row_ptr[n_rows] = nnz > e)
    int64_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (row_ptr[mid] <= e) lo = mid;
      else hi = mid;
    }
    int64_t row = lo, next = row_ptr[row + 1];
    double x[8];
    double xx = load_x_row(X, row, ld, k, g, x);
    double run = 0.0;  // weighted ratings of `row` this group has seen
    for (; e < e_end; e += 16) {
      const int64_t mine = e + g;
      const int32_t c = mine < e_end ? col[mine] : -1;
      const float v = mine < e_end ? val[mine] : 0.f;
      for (int j0 = 0; j0 < 16 && e + j0 < e_end; j0 += 4) {
        float4 y0[4], y1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // the four gathers first: independent of the row walk
          const int32_t cj = __shfl(c, j0 + u, 16);
          const bool ok = Y != nullptr && cj >= 0 && cj < n_cols;
          y0[u] = y1[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (ok && 4 * g < k)
            y0[u] = *reinterpret_cast<const float4*>(Y + (int64_t)cj * ld + 4 * g);
          if (ok && 4 * g + 64 < k)
            y1[u] = *reinterpret_cast<const float4*>(Y + (int64_t)cj * ld + 4 * g + 64);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t ee = e + j0 + u;
          const int32_t cj = __shfl(c, j0 + u, 16);
          const double r = (double)__shfl(v, j0 + u, 16);
          if (ee < e_end) {
            while (ee >= next && row + 1 < n_rows) {
              reg += run * xx;
              run = 0.0;
              ++row;
              next = row_ptr[row + 1];
              xx = load_x_row(X, row, ld, k, g, x);
            }
            cnt += 1.0;
            if (r > 0.0) pos += 1.0;
            if (!implicit || r > 0.0) run += 1.0;
            if (Y != nullptr && cj >= 0 && cj < n_cols) {
              const int d0 = 4 * g;
              double s = 0.0;
              if (d0 < k) s += x[0] * (double)y0[u].x;
              if (d0 + 1 < k) s += x[1] * (double)y0[u].y;
              if (d0 + 2 < k) s += x[2] * (double)y0[u].z;
              if (d0 + 3 < k) s += x[3] * (double)y0[u].w;
              if (d0 + 64 < k) s += x[4] * (double)y1[u].x;
              if (d0 + 65 < k) s += x[5] * (double)y1[u].y;
              if (d0 + 66 < k) s += x[6] * (double)y1[u].z;
              if (d0 + 67 < k) s += x[7] * (double)y1[u].w;
#pragma unroll
              for (int msk = 8; msk >= 1; msk >>= 1) s += shfl_xor_f64(s, msk);
              double term;
              if (implicit) {
                const double conf = 1.0 + alpha * fabs(r);
                const double d = (r > 0.0 ? 1.0 : 0.0) - s;
                term = conf * d * d - s * s;
              } else {
                const double d = r - s;
                term = d * d;
              }
              data += term;
              sabs += fabs(term);
            }
          }
        }
      }
    }
    reg += run * xx;
  }
  if (g == 0) {
    sm[0 * 16 + grp] = data;
    sm[1 * 16 + grp] = sabs;
    sm[2 * 16 + grp] = reg;
    sm[3 * 16 + grp] = cnt;
    sm[4 * 16 + grp] = pos;
  }
  __syncthreads();
  if (threadIdx.x < kObjOut) {
    double a = sm[threadIdx.x * 16];
    for (int q = 1; q < 16; ++q) a += sm[threadIdx.x * 16 + q];
    partial[(int64_t)kObjOut * blockIdx.x + threadIdx.x] = a;
  }
}

// partial[block][kp x kp], kp = 16 T: the block's rows of F^T F.  Lane l of a wave holds, for
// an instruction over table rows r .. r + 3, A[i = l & 15][kk = l >> 4] = F[r + kk][16 ta + i]
// and B[kk][j = l & 15] = F[r + kk][16 tb + j]; its four results are D[row = (l >> 4) + 4 v]
// [col = l & 15], v = 0 .. 3 (the f64 form's own C / D map).
template <int T>
__global__ __launch_bounds__(256) void gram_f64_kernel(const float* __restrict__ F, int64_t n,
                                                       int ld, int k, int64_t rows_per_block,
                                                       double* __restrict__ partial) {
  constexpr int TA = (T + 3) / 4;  // 16-row bands of the output per wave
  constexpr int kp = 16 * T;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c = lane & 15, q = lane >> 4;
  if (wave >= T) return;  // wave-uniform: this wave owns no band
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  double4_t acc[TA][T];
#pragma unroll
  for (int i = 0; i < TA; ++i)
#pragma unroll
    for (int t = 0; t < T; ++t) acc[i][t] = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int64_t r = r0; r < r1; r += 4) {
    const int64_t row = r + q;
    const bool in = row < r1;
    const float* __restrict__ fr = F + (in ? row : r0) * ld;
    double fb[T], fa[TA];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int cc = 16 * t + c;
      fb[t] = (in && cc < k) ? (double)fr[cc] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      const int cc = 16 * (wave + 4 * i) + c;
      fa[i] = (in && cc < k) ? (double)fr[cc] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[i][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[t], acc[i][t], 0, 0, 0);
  }
  double* __restrict__ out = partial + (int64_t)blockIdx.x * kp * kp;
#pragma unroll
  for (int i = 0; i < TA; ++i) {
    const int ta = wave + 4 * i;
    if (ta < T) {
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v)
          out[(int64_t)(16 * ta + q + 4 * v) * kp + 16 * t + c] = acc[i][t][v];
    }
  }
}

// G[a k + b] = sum over blocks, ascending, of partial[block][a kp + b]; written to g_ws and,
// when set, to g_user.
__global__ __launch_bounds__(256) void gram_fold_kernel(const double* __restrict__ partial,
                                                        int64_t nb, int kp, int k,
                                                        double* __restrict__ g_ws,
                                                        double* __restrict__ g_user) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= k * k) return;
  const int a = idx / k, b = idx - a * k;
  double s = 0.0;
  for (int64_t blk = 0; blk < nb; ++blk) s += partial[blk * kp * kp + (int64_t)a * kp + b];
  g_ws[idx] = s;
  if (g_user) g_user[idx] = s;
}

// <ga, gb>_F over k x k, one block: each thread its elements ascending, then the tree.
__global__ __launch_bounds__(256) void gram_dot_kernel(const double* __restrict__ ga,
                                                       const double* __restrict__ gb, int kk,
                                                       double* __restrict__ out) {
  __shared__ double sm[256];
  double a = 0.0;
  for (int idx = threadIdx.x; idx < kk; idx += 256) a += ga[idx] * gb[idx];
  a = block_tree_sum(a, sm);
  if (threadIdx.x == 0) out[0] = a;
}

static inline int64_t obj_blocks(int64_t nnz) { return (nnz + kObjSpan - 1) / kObjSpan; }

// Rows per block (a multiple of 4) and blocks of the Gram of an n-row table; both depend on n
// alone, so the summation order does too.
static inline int64_t gram_rows_per_block(int64_t n) {
  int64_t nb = (n + kGramMinRows - 1) / kGramMinRows;
  if (nb > kGramMaxBlocks) nb = kGramMaxBlocks;
  if (nb < 1) nb = 1;
  return ((n + nb - 1) / nb + 3) / 4 * 4;
}
static inline int64_t gram_blocks(int64_t n) {
  const int64_t rpb = gram_rows_per_block(n);
  return n > 0 ? (n + rpb - 1) / rpb : 0;
}
static inline int gram_tiles(int k) { return (k + 15) / 16; }

static size_t gram_partial_doubles(int64_t n, int k) {
  const size_t kp = 16 * (size_t)gram_tiles(k);
  return (size_t)gram_blocks(n) * kp * kp;
}
// The same for any table of at most n rows: gram_blocks(m) <= min(kGramMaxBlocks,
// ceil(m / kGramMinRows)), which is monotone in m (gram_blocks itself is not).
static size_t gram_partial_doubles_bound(int64_t n, int k) {
  const size_t kp = 16 * (size_t)gram_tiles(k);
  int64_t nb = (n + kGramMinRows - 1) / kGramMinRows;
  if (nb > kGramMaxBlocks) nb = kGramMaxBlocks;
  return (size_t)nb * kp * kp;
}

static int launch_gram(const float* F, int64_t n, int ld, int k, double* partial, double* g_ws,
                       double* g_user, hipStream_t st) {
  const int T = gram_tiles(k);
  const int64_t rpb = gram_rows_per_block(n), nb = gram_blocks(n);
  const unsigned grid = (unsigned)nb;
  switch (T) {
#define ALS_GRAM_CASE(t)                                                          \
  case t:                                                                         \
    gram_f64_kernel<t><<<grid, 256, 0, st>>>(F, n, ld, k, rpb, partial);           \
    break;
    ALS_GRAM_CASE(1) ALS_GRAM_CASE(2) ALS_GRAM_CASE(3) ALS_GRAM_CASE(4)
    ALS_GRAM_CASE(5) ALS_GRAM_CASE(6) ALS_GRAM_CASE(7) ALS_GRAM_CASE(8)
#undef ALS_GRAM_CASE
    default:
      set_error("als_gram_dot_f64: rank %d unsupported", k);
      return ALS_EUNSUPPORTED;
  }
  ALS_LAUNCH_CHECK();
  gram_fold_kernel<<<(unsigned)((k * k + 255) / 256), 256, 0, st>>>(partial, nb, 16 * T, k, g_ws,
                                                                   g_user);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // namespace als

using namespace als;

extern "C" {

int32_t als_objective_span(void) { return kObjSpan; }

size_t als_objective_workspace_bytes(int64_t nnz, int64_t n_rows, int32_t k) {
  if (nnz < 0) nnz = 0;
  if (n_rows < 0) n_rows = 0;
  if (k < 1) k = 1;
  if (k > 128) k = 128;
  const size_t side = align_up(sizeof(double) * kObjOut * (size_t)obj_blocks(nnz));
  // both tables' partial Grams (each at most n_rows rows) and their folded k x k forms
  const size_t gram = 2 * align_up(sizeof(double) * gram_partial_doubles_bound(n_rows, k)) +
                      2 * align_up(sizeof(double) * (size_t)k * k);
  return (side > gram ? side : gram) + 256;
}

int als_objective_side(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t nnz,
                       int32_t n_rows, int32_t n_cols, const float* X, const float* Y, int32_t ld,
                       int32_t k, int implicit, float alpha, double* out, void* ws,
                       size_t ws_bytes, void* stream) {
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_objective_side: rank %d outside [1, 128]",
              k);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_objective_side: bad ld %d for k %d", ld, k);
  ALS_REQUIRE(nnz >= 0 && n_rows >= 0 && n_cols >= 0, ALS_EINVAL,
              "als_objective_side: negative size");
  ALS_REQUIRE(alpha >= 0.f, ALS_EINVAL, "als_objective_side: alpha < 0");
  hipStream_t st = as_stream(stream);
  if (nnz == 0 || n_rows == 0) {
    if (out) ALS_HIP(hipMemsetAsync(out, 0, kObjOut * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(row_ptr && col && val && X && out, ALS_EINVAL, "als_objective_side: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(Y) & 15) == 0,
              ALS_EINVAL, "als_objective_side: factors not 16-byte aligned");
  const int64_t nb = obj_blocks(nnz);
  ALS_REQUIRE(ws && ws_bytes >= align_up(sizeof(double) * kObjOut * (size_t)nb), ALS_EWORKSPACE,
              "als_objective_side: workspace too small");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, ALS_EINVAL,
              "als_objective_side: workspace not 8-byte aligned");
  ALS_REQUIRE(nb <= 0x7fffffff, ALS_EUNSUPPORTED, "als_objective_side: nnz too large");
  double* partial = static_cast<double*>(ws);
  objective_side_kernel<<<(unsigned)nb, 256, 0, st>>>(row_ptr, col, val, nnz, n_rows, n_cols, X, Y,
                                                      ld, k, implicit != 0, (double)alpha,
                                                      partial);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kObjOut><<<1, 256, 0, st>>>(partial, nb, out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

int als_gram_dot_f64(const float* A, int64_t n_a, const float* B, int64_t n_b, int32_t ld,
                     int32_t k, double* out, double* gram_a_out, double* gram_b_out, void* ws,
                     size_t ws_bytes, void* stream) {
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_gram_dot_f64: rank %d outside [1, 128]",
              k);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_gram_dot_f64: bad ld %d for k %d", ld, k);
  ALS_REQUIRE(n_a >= 0 && n_b >= 0, ALS_EINVAL, "als_gram_dot_f64: negative size");
  hipStream_t st = as_stream(stream);
  const size_t kk = (size_t)k * k;
  if (n_a == 0 || n_b == 0) {  // an empty table's Gram is zero, and so is the product
    if (out) ALS_HIP(hipMemsetAsync(out, 0, sizeof(double), st));
    if (n_a == 0 && gram_a_out) ALS_HIP(hipMemsetAsync(gram_a_out, 0, kk * sizeof(double), st));
    if (n_b == 0 && gram_b_out) ALS_HIP(hipMemsetAsync(gram_b_out, 0, kk * sizeof(double), st));
    if (n_a == 0 && n_b == 0) return ALS_OK;
    if (!(n_a == 0 ? gram_b_out : gram_a_out)) return ALS_OK;  // nothing else asked for
  }
  ALS_REQUIRE((n_a == 0 || A) && (n_b == 0 || B) && out, ALS_EINVAL,
              "als_gram_dot_f64: null pointer");
  const size_t pa = align_up(sizeof(double) * gram_partial_doubles(n_a, k));
  const size_t pb = align_up(sizeof(double) * gram_partial_doubles(n_b, k));
  const size_t need = pa + pb + 2 * align_up(sizeof(double) * kk);
  ALS_REQUIRE(ws && ws_bytes >= need, ALS_EWORKSPACE, "als_gram_dot_f64: workspace too small");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7) == 0, ALS_EINVAL,
              "als_gram_dot_f64: workspace not 8-byte aligned");
  char* base = static_cast<char*>(ws);
  double* part_a = reinterpret_cast<double*>(base);
  double* part_b = reinterpret_cast<double*>(base + pa);
  double* g_a = reinterpret_cast<double*>(base + pa + pb);
  double* g_b = reinterpret_cast<double*>(base + pa + pb + align_up(sizeof(double) * kk));
  if (n_a > 0) {
    const int rc = launch_gram(A, n_a, ld, k, part_a, g_a, gram_a_out, st);
    if (rc != ALS_OK) return rc;
  }
  if (n_b > 0) {
    const int rc = launch_gram(B, n_b, ld, k, part_b, g_b, gram_b_out, st);
    if (rc != ALS_OK) return rc;
  }
  if (n_a > 0 && n_b > 0) {
    gram_dot_kernel<<<1, 256, 0, st>>>(g_a, g_b, (int)kk, out);
    ALS_LAUNCH_CHECK();
  }
  return ALS_OK;
}

}  // extern "C"
