// K13 — nonnegative rows: the normal equations of K7 solved by Spark's NNLS
// (mllib/optimization/NNLS.scala: projected gradient with conjugate-gradient directions)
// instead of Cholesky (als_nnls_rows, ABI 9).
//
// Spark's `nonnegative` only swaps the per-row solver, so the input, the sums and the
// regularisation are als_fold_in's; one entry point serves a training half-sweep (a
// RatingBlock's row_ptr / col / val have the ragged layout) and a fold-in.
//
//   order    Rows run longest first: a key per row (an upper bound of the degree minus the
//            degree), the radix sort of K1, and the solve launch walks the sorted list.
//   partial  A row with more than `chunk` ratings is cut into chunk-rating tasks (slot
//            numbers from an exclusive scan of the rows' task counts).  One workgroup per
//            task forms the task's Gram exactly as a short row does and writes its fp64
//            accumulators, b and the two counts to the task's workspace slot.
//   solve    One 256-thread workgroup per row.  A short row forms its Gram in place (the
//            code shared with K7 through row_system.h: 32 ratings staged at a time, thread
//            (a, b) of a 16 x 16 grid owns the entries (a + 16 p, b + 16 q), q <= p, fp64,
//            rating order); a long row sums its slots in slot order.  YtY and reg * n go on
//            there, and A is written to LDS as a full symmetric KP x KP fp64 matrix.
//   nnls     G = 256 / KP threads share a row of A; thread i * G owns element i of x, dir,
//            lastDir, grad, res and b in registers, and x and the direction are published
//            in LDS for the matrix-vector products.  Every scalar that decides control flow
//            (step, dstep, ndir, nx, ngrad, the wall clamp, the wall flag) is reduced
//            inside each wavefront by xor-shuffles, the four wavefront values go through
//            LDS, and after one barrier EVERY thread adds the same four words in the same
//            order: all 256 threads branch on the same bits, so no barrier sits inside
//            divergent control flow.  The loop is bounded by iterMax = max(400, 20 k).
// The result is deterministic: nothing depends on which workgroup runs when.
#include <algorithm>

#include "row_system.h"

namespace als {

// Dynamic LDS of one block.  A (KP rows of LDA doubles) comes first; the gather buffer of the
// Gram stage aliases its head (32 * KP floats <= KP * 32 doubles <= A).
template <int NB>
struct NnShape {
  static constexpr int KP = 16 * NB;
  static constexpr int G = kRowThreads / KP;  // threads per row of A
  static constexpr int LDA = KP + G;         // 32 lanes of a ds_read_b64 hit 32 different banks
  static constexpr int JT = KP / G;          // columns per thread
  static constexpr int NACC = NB * (NB + 1) / 2;
  static constexpr int A_DOUBLES = KP * LDA;
  // A | x | dir | wa | wb | 4 reduction sites of [4 waves][4] | col | counts, flags
  static constexpr int DOUBLES = A_DOUBLES + 2 * KP + 2 * kRowBatch + 4 * 16;
  static constexpr int BYTES = DOUBLES * 8 + kRowBatch * 4 + 8 * 4;
  // one task's workspace slot: the accumulators and b in thread layout, then n and n+
  static constexpr int64_t SLOT_DOUBLES = (int64_t)(NACC + 1) * kRowThreads + 2;
};

static inline int64_t nn_slot_doubles(int kp) {
  const int nb = kp / 16;
  return (int64_t)(nb * (nb + 1) / 2 + 1) * kRowThreads + 2;
}

struct NnSmem {
  double* A;
  float* ybuf;
  double* sx;
  double* sd;
  double* swa;
  double* swb;
  double* sred;  // [4 sites][4 waves][4]
  int* scol;
  int* scnt;  // [0] n, [1] n+, [4..7] wall flags
};

template <int NB>
__device__ __forceinline__ NnSmem nn_smem(void* base) {
  using S = NnShape<NB>;
  NnSmem m;
  m.A = reinterpret_cast<double*>(base);
  m.ybuf = reinterpret_cast<float*>(base);
  m.sx = m.A + S::A_DOUBLES;
  m.sd = m.sx + S::KP;
  m.swa = m.sd + S::KP;
  m.swb = m.swa + kRowBatch;
  m.sred = m.swb + kRowBatch;
  m.scol = reinterpret_cast<int*>(m.sred + 4 * 16);
  m.scnt = m.scol + kRowBatch;
  return m;
}

// ---- schedule: sort keys, task counts ----
__global__ __launch_bounds__(256) void nnls_keys_kernel(const int64_t* __restrict__ row_ptr,
                                                        int64_t n_rows, int64_t chunk,
                                                        uint32_t key_max,
                                                        uint32_t* __restrict__ keys,
                                                        int32_t* __restrict__ rows,
                                                        int32_t* __restrict__ ntasks) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= n_rows;
       r += (int64_t)gridDim.x * 256) {
    if (r == n_rows) {
      ntasks[r] = 0;  // the scan leaves the total here
      continue;
    }
    int64_t deg = row_ptr[r + 1] - row_ptr[r];
    if (deg < 0) deg = 0;
    keys[r] = key_max - (uint32_t)std::min<int64_t>(deg, (int64_t)key_max);
    rows[r] = (int32_t)r;
    ntasks[r] = deg > chunk ? (int32_t)((deg + chunk - 1) / chunk) : 0;
  }
}

// ---- partial: one task of a long row -> its slot ----
template <int NB, bool IMPLICIT>
__global__ __launch_bounds__(kRowThreads) void nnls_partial_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_rows, const float* __restrict__ Y, int64_t n_src,
    int ld, int k, float alpha, int64_t chunk, const int32_t* __restrict__ slot_begin,
    int64_t max_slots, double* __restrict__ slots) {
  using S = NnShape<NB>;
  extern __shared__ float4 nn_smem_raw[];
  const NnSmem m = nn_smem<NB>(nn_smem_raw);
  const int t = threadIdx.x;
  // a workspace smaller than als_nnls_workspace_bytes asks for holds fewer slots than
  // there are tasks: the rows past it are summed serially by the solve launch instead
  int64_t total = slot_begin[n_rows];
  if (total > max_slots) total = max_slots;
  for (int64_t task = blockIdx.x; task < total; task += gridDim.x) {
    // the row r with slot_begin[r] <= task < slot_begin[r + 1] (the same words in every thread)
    int64_t lo = 0, hi = n_rows;  // first index in (lo, hi] whose slot_begin > task
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)slot_begin[mid] > task) hi = mid; else lo = mid;
    }
    const int64_t row = lo;
    const int64_t j = task - slot_begin[row];
    const int64_t pb = row_ptr[row] + j * chunk;
    const int64_t pe = std::min<int64_t>(pb + chunk, row_ptr[row + 1]);
    double acc[S::NACC];
#pragma unroll
    for (int i = 0; i < S::NACC; ++i) acc[i] = 0.0;
    double bacc = 0.0;
    int n_used = 0, n_pos = 0;
    row_gram<NB, IMPLICIT>(pb, pe, col, val, Y, n_src, ld, k, alpha, m.scol, m.swa, m.swb, m.ybuf,
                           acc, bacc, n_used, n_pos);
    double* const sl = slots + task * S::SLOT_DOUBLES;
#pragma unroll
    for (int i = 0; i < S::NACC; ++i) sl[i * kRowThreads + t] = acc[i];
    sl[S::NACC * kRowThreads + t] = bacc;
    if (t == 0) {
      sl[(S::NACC + 1) * kRowThreads] = (double)n_used;
      sl[(S::NACC + 1) * kRowThreads + 1] = (double)n_pos;
    }
  }
}

// ---- the workgroup-wide reductions: every thread returns the same bits ----
template <int NV>
__device__ __forceinline__ void nn_block_sum(double (&v)[NV], double* site) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < NV; ++n) {
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v[n] += shfl_xor_f64(v[n], msk);
    if (lane == 0) site[wave * 4 + n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < NV; ++n) v[n] = ((site[n] + site[4 + n]) + site[8 + n]) + site[12 + n];
}

__device__ __forceinline__ double nn_block_min(double v, double* site) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int msk = 32; msk >= 1; msk >>= 1) v = fmin(v, shfl_xor_f64(v, msk));
  if (lane == 0) site[wave * 4] = v;
  __syncthreads();
  return fmin(fmin(site[0], site[4]), fmin(site[8], site[12]));
}

// Row i of A times v, for the G threads of the row: each takes every G-th column, four
// running sums, then the G lanes add up by xor-shuffles (all G return the same bits).
template <int NB>
__device__ __forceinline__ double nn_rowdot(const double* __restrict__ arow,
                                            const double* __restrict__ v, int g) {
  using S = NnShape<NB>;
  double s;
  if constexpr (S::JT >= 4) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int c = 0; c < S::JT; c += 4) {
      s0 = fma(arow[S::G * c], v[g + S::G * c], s0);
      s1 = fma(arow[S::G * (c + 1)], v[g + S::G * (c + 1)], s1);
      s2 = fma(arow[S::G * (c + 2)], v[g + S::G * (c + 2)], s2);
      s3 = fma(arow[S::G * (c + 3)], v[g + S::G * (c + 3)], s3);
    }
    s = (s0 + s1) + (s2 + s3);
  } else {
    s = arow[0] * v[g];
  }
#pragma unroll
  for (int msk = S::G / 2; msk >= 1; msk >>= 1) s += shfl_xor_f64(s, msk);
  return s;
}

__device__ __forceinline__ bool nn_stop(double step, double ndir, double nx) {
  return (step != step) || step < 1e-7 || step > 1e40 || ndir < 1e-12 * nx || ndir < 1e-32;
}

// ---- solve: one row per workgroup ----
template <int NB, bool IMPLICIT>
__global__ __launch_bounds__(kRowThreads) void nnls_solve_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_rows, const int32_t* __restrict__ order,
    const float* __restrict__ Y, int64_t n_src, int ld, int k, float reg, float alpha,
    const double* __restrict__ yty, const int32_t* __restrict__ slot_begin, int64_t max_slots,
    const double* __restrict__ slots, float* __restrict__ X, int ld_out,
    int32_t* __restrict__ n_used_out, int32_t* __restrict__ iters_out) {
  using S = NnShape<NB>;
  constexpr int KP = S::KP, G = S::G, LDA = S::LDA;
  extern __shared__ float4 nn_smem_raw[];
  const NnSmem m = nn_smem<NB>(nn_smem_raw);
  const int t = threadIdx.x;
  const int ta = t >> 4, tb = t & 15;
  const int lane = t & 63, wave = t >> 6;
  const int ri = t / G, g = t % G;      // this thread's row of A and its column phase
  const bool own = g == 0 && ri < k;    // thread ri * G owns element ri of the vectors
  const double* const arow = m.A + ri * LDA + g;
  const int iter_max = 20 * k > 400 ? 20 * k : 400;

  for (int64_t w = blockIdx.x; w < n_rows; w += gridDim.x) {
    const int64_t row = order ? (int64_t)order[w] : w;
    const int64_t pb = row_ptr[row], pe = row_ptr[row + 1];
    double acc[S::NACC];
#pragma unroll
    for (int i = 0; i < S::NACC; ++i) acc[i] = 0.0;
    double bacc = 0.0;
    int n_used = 0, n_pos = 0;
    int64_t sb = 0, se = 0;
    if (slot_begin && (int64_t)slot_begin[row + 1] <= max_slots) {
      sb = slot_begin[row];
      se = slot_begin[row + 1];
    }
    if (se > sb) {  // a long row: its tasks' partials, in slot order
      double cn = 0.0, cp = 0.0;
      for (int64_t s = sb; s < se; ++s) {
        const double* const sl = slots + s * S::SLOT_DOUBLES;
#pragma unroll
        for (int i = 0; i < S::NACC; ++i) acc[i] += sl[i * kRowThreads + t];
        bacc += sl[S::NACC * kRowThreads + t];
        cn += sl[(S::NACC + 1) * kRowThreads];
        cp += sl[(S::NACC + 1) * kRowThreads + 1];
      }
      n_used = (int)cn;
      n_pos = (int)cp;
    } else {
      row_gram<NB, IMPLICIT>(pb, pe, col, val, Y, n_src, ld, k, alpha, m.scol, m.swa, m.swb,
                             m.ybuf, acc, bacc, n_used, n_pos);
    }
    if (t == 0) {
      m.scnt[0] = n_used;
      m.scnt[1] = n_pos;
    }
    if (t < KP) m.sd[t] = bacc;  // b: from the Gram's thread t to the owner of element t
    __syncthreads();
    const int n_all = m.scnt[0];
    const double lam_n = (double)reg * (double)(IMPLICIT ? m.scnt[1] : n_all);
    float* const xr = X + row * (int64_t)ld_out;
    if (n_used_out && t == 0) n_used_out[row] = n_all;
    if (n_all == 0) {  // no used entry: b = 0, the solver's answer at its first test
      for (int c = t; c < ld_out; c += kRowThreads) xr[c] = 0.f;
      if (iters_out && t == 0) iters_out[row] = 0;
      __syncthreads();  // scnt and sd are rewritten by the next row
      continue;
    }

    // accumulators -> the full symmetric matrix; rows and columns >= k stay zero
#pragma unroll
    for (int p = 0; p < NB; ++p) {
#pragma unroll
      for (int q = 0; q <= p; ++q) {
        const int i = ta + 16 * p, j = tb + 16 * q;
        if (j <= i) {
          double a = acc[p * (p + 1) / 2 + q];
          if (i < k) {
            if (IMPLICIT) a += yty[i * (i + 1) / 2 + j];
            if (i == j) a += lam_n;
          }
          m.A[i * LDA + j] = a;
          m.A[j * LDA + i] = a;
        }
      }
    }
    const double bi = own ? m.sd[ri] : 0.0;
    double x = 0.0, last_dir = 0.0, last_norm = 0.0;
    int last_wall = 0, iterno = 0;
    __syncthreads();  // A complete, b read
    if (t < KP) m.sx[t] = 0.0;
    __syncthreads();

    while (iterno < iter_max) {
      // res = A x - b, the projected gradient
      const double ax = nn_rowdot<NB>(arow, m.sx, g);
      const double res = own ? ax - bi : 0.0;
      const double grad = (res > 0.0 && x == 0.0) ? 0.0 : res;
      if (own) m.sd[ri] = grad;
      __syncthreads();
      const double ag = nn_rowdot<NB>(arow, m.sd, g);
      double r1[4] = {grad * grad, x * x, grad * res, own ? ag * grad : 0.0};
      nn_block_sum<4>(r1, m.sred);
      const double ngrad = r1[0], nx = r1[1];
      double step = r1[2] / (r1[3] + 1e-20);
      double dir = grad, ndir = ngrad;
      if (iterno > last_wall + 1) {  // uniform: both are the same in every thread
        const double cg = ngrad / last_norm;
        const double d2 = own ? grad + cg * last_dir : 0.0;
        if (own) m.sd[ri] = d2;
        __syncthreads();
        const double ad = nn_rowdot<NB>(arow, m.sd, g);
        double r2[3] = {d2 * res, own ? ad * d2 : 0.0, d2 * d2};
        nn_block_sum<3>(r2, m.sred + 16);
        const double dstep = r2[0] / (r2[1] + 1e-20);
        if (!nn_stop(dstep, r2[2], nx)) {  // else: the CG step is rejected, dir stays grad
          dir = d2;
          ndir = r2[2];
          step = dstep;
        }
      }
      if (nn_stop(step, ndir, nx)) break;  // the same bits in every thread
      // the wall: no coordinate may go below zero
      const double cand = (own && step * dir > x) ? x / dir : __builtin_huge_val();
      step = fmin(step, nn_block_min(cand, m.sred + 32));
      bool hit = false;
      if (own) {
        if (step * dir > x * (1.0 - 1e-14)) {
          x = 0.0;
          hit = true;
        } else {
          x -= step * dir;
        }
        m.sx[ri] = x;
      }
      const bool wave_hit = __ballot(hit) != 0;
      if (lane == 0) m.scnt[4 + wave] = wave_hit ? 1 : 0;
      __syncthreads();  // x published, flags visible
      if (m.scnt[4] | m.scnt[5] | m.scnt[6] | m.scnt[7]) last_wall = iterno;
      ++iterno;
      last_dir = dir;
      last_norm = ngrad;
    }
    if (own) xr[ri] = (float)x;
    for (int c = k + t; c < ld_out; c += kRowThreads) xr[c] = 0.f;
    if (iters_out && t == 0) iters_out[row] = iterno;
    __syncthreads();  // A, sx, sd, scnt and the reduction sites are rewritten by the next row
  }
}

struct NnWs {
  uint32_t* keys_in;
  int32_t* rows_in;
  uint32_t* keys_out;
  int32_t* order;
  int32_t* slot_begin;
  void* sort_ws;
  size_t sort_bytes;
  void* scan_ws;
  size_t scan_bytes;
  double* slots;
  int64_t max_slots;
};

static inline int64_t nn_max_slots(int64_t n_rows, int64_t nnz, int64_t chunk) {
  // a row of d > chunk ratings has ceil(d / chunk) <= d / chunk + 1 tasks, and fewer than
  // nnz / chunk rows are that long
  const int64_t full = nnz / chunk;
  return full + std::min<int64_t>(n_rows, full);
}

// ms < 0: the slots take whatever the workspace has left after the fixed part
template <class AR>
static void nn_layout(AR& a, int64_t n_rows, int kp, int64_t ms, NnWs* out) {
  const size_t sort_bytes = radix_workspace_bytes(n_rows);
  const size_t scan_bytes = scan_workspace_bytes(n_rows + 1);
  auto keys_in = a.template take<uint32_t>(n_rows);
  auto rows_in = a.template take<int32_t>(n_rows);
  auto keys_out = a.template take<uint32_t>(n_rows);
  auto order = a.template take<int32_t>(n_rows);
  auto slot_begin = a.template take<int32_t>(n_rows + 1);
  auto sort_ws = a.template take<char>(sort_bytes);
  auto scan_ws = a.template take<char>(scan_bytes);
  if (ms < 0) ms = (int64_t)(a.left() / ((size_t)nn_slot_doubles(kp) * 8));
  auto slots = a.template take<double>((size_t)(ms * nn_slot_doubles(kp)));
  if (out) {
    out->keys_in = (uint32_t*)keys_in;
    out->rows_in = (int32_t*)rows_in;
    out->keys_out = (uint32_t*)keys_out;
    out->order = (int32_t*)order;
    out->slot_begin = (int32_t*)slot_begin;
    out->sort_ws = (void*)sort_ws;
    out->sort_bytes = sort_bytes;
    out->scan_ws = (void*)scan_ws;
    out->scan_bytes = scan_bytes;
    out->slots = (double*)slots;
    out->max_slots = ms;
  }
}

// ArenaSize::take returns void: a shim with Arena's shape
struct NnArenaSize {
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    off += align_up(count * sizeof(T));
    return nullptr;
  }
  size_t left() const { return 0; }
};
struct NnArena {
  Arena ar;
  bool ok = true;
  NnArena(void* b, size_t c) : ar(b, c) {}
  template <class T>
  T* take(size_t count) {
    T* p = ar.take<T>(count);
    if (!p) ok = false;
    return p;
  }
  size_t left() const { return ar.cap > ar.off ? ar.cap - ar.off : 0; }
};

}  // namespace als

using namespace als;

extern "C" {

size_t als_nnls_workspace_bytes(int64_t n_rows, int64_t nnz, int32_t k, int32_t chunk) {
  if (n_rows <= 0 || nnz < 0 || k < 1 || k > kRowMaxRank || chunk < 1) return 0;
  NnArenaSize a;
  nn_layout(a, n_rows, als_k_pad(k), nn_max_slots(n_rows, nnz, chunk), nullptr);
  return a.off + 256;
}

int als_nnls_rows(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows,
                  const float* Y_src, int64_t n_src, int32_t ld, int32_t k, float reg,
                  int implicit, float alpha, const double* yty_packed, int32_t chunk,
                  float* X_out, int32_t ld_out, int32_t* n_used_out, int32_t* iters_out, void* ws,
                  size_t ws_bytes, void* stream) {
  if (int rc = row_check_args("als_nnls_rows", k, ld, n_rows, n_src, reg, alpha, implicit,
                              yty_packed))
    return rc;
  ALS_REQUIRE(ld_out >= k && ld_out % 4 == 0, ALS_EINVAL,
              "als_nnls_rows: ld_out %d must be >= k and a multiple of 4", ld_out);
  ALS_REQUIRE(chunk >= 1, ALS_EINVAL, "als_nnls_rows: chunk %d must be >= 1", chunk);
  if (n_rows == 0) return ALS_OK;
  ALS_REQUIRE(row_ptr && col && val && X_out, ALS_EINVAL, "als_nnls_rows: null pointer");
  if (int rc = row_check_source("als_nnls_rows", n_src, Y_src, X_out)) return rc;
  ALS_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_nnls_rows: workspace null or not 16-byte aligned");
  const int kp = als_k_pad(k);
  NnWs W;
  NnArena ar(ws, ws_bytes);
  nn_layout(ar, n_rows, kp, -1, &W);
  ALS_REQUIRE(ar.ok, ALS_EWORKSPACE, "als_nnls_rows: workspace of %zu bytes too small", ws_bytes);
  hipStream_t st = as_stream(stream);

  // longest first; the rows' task counts -> slot numbers
  const int bits = 31;
  const uint32_t key_max = 0x7fffffffu;  // longer rows tie at key 0
  const unsigned kg = (unsigned)std::min<int64_t>((n_rows + 256) / 256, 4096);
  nnls_keys_kernel<<<kg, 256, 0, st>>>(row_ptr, n_rows, (int64_t)chunk, key_max, W.keys_in,
                                       W.rows_in, W.slot_begin);
  ALS_LAUNCH_CHECK();
  const int32_t* order = nullptr;
  if (n_rows > 1) {
    int rc = radix_sort_pairs(W.keys_in, W.rows_in, W.keys_out, W.order, n_rows, bits, W.sort_ws,
                              W.sort_bytes, st);
    if (rc) return rc;
    order = W.order;
  }
  const int32_t* slot_begin = nullptr;
  if (W.max_slots > 0) {
    int rc = scan_exclusive_i32(W.slot_begin, W.slot_begin, n_rows + 1, W.scan_ws, W.scan_bytes,
                                st);
    if (rc) return rc;
    slot_begin = W.slot_begin;
  }

  const unsigned grid = (unsigned)std::min<int64_t>(n_rows, kRowMaxBlocks);
  const unsigned pgrid = (unsigned)std::min<int64_t>(W.max_slots, kRowMaxBlocks);
  return row_dispatch(kp / 16, implicit, [&](auto nbc, auto imp) -> int {
    constexpr int NB = decltype(nbc)::value;
    constexpr auto partial = &nnls_partial_kernel<NB, decltype(imp)::value>;
    constexpr auto solve = &nnls_solve_kernel<NB, decltype(imp)::value>;
    const int lds = NnShape<NB>::BYTES;
    if (pgrid > 0) {
      ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(partial),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      partial<<<pgrid, kRowThreads, lds, st>>>(row_ptr, col, val, n_rows, Y_src, n_src, ld, k,
                                               alpha, (int64_t)chunk, slot_begin, W.max_slots,
                                               W.slots);
      ALS_LAUNCH_CHECK();
    }
    ALS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(solve),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    solve<<<grid, kRowThreads, lds, st>>>(row_ptr, col, val, n_rows, order, Y_src, n_src, ld, k,
                                          reg, alpha, yty_packed, slot_begin, W.max_slots, W.slots,
                                          X_out, ld_out, n_used_out, iters_out);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  });
}

}  // extern "C"
