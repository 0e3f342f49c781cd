// K5 — recommendForAll: blocked U.V^T on the matrix cores with a fused,
// bounded per-row top-k.  The n_q x n_v score matrix is never materialised.
//
// Replaces ALSModel.recommendForAll (upstream Spark >= 2.2: blockify at 4096
// rows, crossJoin, sgemm per block pair, bounded priority queue,
// TopByKeyAggregator merge) and mllib recommendProductsForUsers.  The
// reference's own top-k is `predictAll` over one user's unrated movies then
// `takeOrdered(20, key=-pred)` (RecommenderSystem.py:229-247).
//
// Scores on the f16 matrix cores with fp32-grade products (the split scheme
// of the Gram in gram_solve.hip): q and v are scaled by powers of two (from
// max |Q| and max |V|) and carried as f16 hi + lo, hi = f16_rn(t),
// lo = f16_rn(t - hi); <q, v> = hi.hi + hi.lo + lo.hi accumulated in fp32 by
// v_mfma_f32_16x16x32_f16 (~2^-21 relative to |q||v| per product, below the
// rounding of Spark's fp32 sgemm).  V is split once per call into f16 planes
// (topk_split_table_kernel: row r = [hi of dims 0..KQ) | lo of dims 0..KQ)]),
// so a staged tile row is copied as is and every B operand is one
// ds_read_b128.  The query rows are split in registers once per workgroup.
//
// Workgroup = NW wavefronts x RG row groups = 16 NW RG query rows.  The workgroup
// sweeps V in tiles double-buffered in LDS (one barrier per tile, the next tile's
// LDS-DMA pieces in flight).  V is swept in order of decreasing row norm
// (bucketed; the high-scoring rows come first, so the lists fill with
// near-final entries early), each 16 x 16 score block is filtered against its
// rows' current k-th best score, and the rare survivors are inserted into the
// per-row lists: in registers for top <= 16, sorted in LDS with a
// wave-cooperative insertion above.  Insertions compare (score, V row index)
// exactly, so the sweep order changes the speed, not the result.  Order: score
// descending, ties by ascending index (the build's deterministic tie rule,
// SURVEY Appendix A.6).  Scores are compared in the scaled domain (exact:
// powers of two) and unscaled on output.  An all-zero query row scores 0
// against every V row; its list is the first `top` rows by index.
//
// This file: the host side — the launch choice (list class, wavefronts, row groups, LDS
// bytes), the workspace and the entry points.  The kernels are in headers: topk_split.h
// (the f16 split), topk_prep.h (V's preparation), topk_lists.h (lists, logs, the filter's
// verdict) and topk_sweep.h (the sweep kernel and its launch), which topk_filtered.hip
// instantiates a second time with a row filter.
#include "topk_prep.h"
#include "topk_sweep.h"

#include <algorithm>

namespace als {

constexpr int kLdsBytes = 160 * 1024;  // per CU on gfx950 (one workgroup may use it all)

static int topk_kq(int k) { return k <= 32 ? 32 : (k <= 64 ? 64 : 128); }

// Key logs for kTopR < top <= kTopQ.  (Round 4's quad register lists measured at rank
// 128, top 100 against the LDS lists: 59,047 V rows 70 -> 21 ms, 1,000,000 V rows 456 ->
// 330 ms; the logs replaced them in round 6.)
static bool topk_logs(int top) { return top > kTopR && top <= kTopQ; }

static int topk_nw(int top, bool logs) {
  return logs ? tk_nw(kTopQ) : (top <= kTopR ? tk_nw(1) : tk_nw(0));
}

static size_t topk_split_lds_bytes(int kq, int rg, int top, bool logs) {
  const int nk = kq / 32;
  const int nw = topk_nw(top, logs);
  const bool reg_lists = top <= kTopR || logs;
  const size_t vt = (size_t)tk_vt(nk, reg_lists ? 1 : 0);
  // [nbuf][vt] tile rows of KQ hi halves (kq/8 uint4) | [nbuf][max(vt, 64)] V rows |
  // [2][nw] done flags | [nw][rg][16] slack coefficients | [nw][nk][64] uint4 lo scratch
  const size_t nbuf = (size_t)tk_nbuf();
  const size_t tiles = 16 * nbuf * vt * (size_t)(kq / 8) + 4 * nbuf * std::max<size_t>(vt, 64) + 4 * 2 * nw +
                       4 * 16 * nw * (size_t)rg + 16 * nw * 64 * (size_t)nk;
  if (reg_lists) return tiles + sizeof(float) * nw * (size_t)rg * (256 + 16);
  return tiles + sizeof(uint64_t) * 64 * (size_t)rg * top +
         sizeof(int) * 64 * (size_t)rg;
}

// Row groups per workgroup of the split kernel (0: its lists do not fit the LDS).
// Two groups halve the V traffic per query row, but LDS lists (top > kTopR) of
// two groups must still leave room for two workgroups per CU: the list inserts
// are latency-bound and need the second workgroup (measured, configs[4] top-100
// at rank 128: one 120 KB workgroup per CU 602 ms, two 68 KB ones 480 ms).
// Register lists take two groups (256 query rows per 8-wave workgroup) only when
// that still gives >= 4 workgroups per CU: measured top-10, ML-25M shape (162,541
// users, rank 64) 4.7 ms with two groups, 3.6 ms with one (the tail of 2.5 rounds);
// configs[4] (262,144-user sample, rank 128) 97 ms with two, 151 ms with one.
constexpr int64_t kTkRg2MinRows = 4 * 256 * 256;
static int topk_split_rg(int k, int top, bool logs, int64_t n_q) {
  const int kq = topk_kq(k);
  // register lists and key logs: two row groups on the same condition (the logs keep
  // no list in registers, so two groups' A operands and accumulators fit)
  if ((top <= kTopR || logs) && n_q < kTkRg2MinRows) return 1;
  if (logs) return 2;
  const size_t rg2_limit = top > kTopR ? (size_t)kLdsBytes / 2 : (size_t)kLdsBytes;
  if (topk_split_lds_bytes(kq, 2, top, false) <= rg2_limit) return 2;
  if (topk_split_lds_bytes(kq, 1, top, false) <= (size_t)kLdsBytes) return 1;
  return 0;
}

}  // namespace als

using namespace als;

extern "C" {

static size_t tk_table_bytes(int64_t n_v, int32_t k) {
  return align_up(4 * (size_t)topk_kq(k) * (size_t)(n_v > 0 ? n_v : 0));
}

// Per-row key logs (16 < top <= 128): tk_log_cap keys for every query
// row of one launch's blocks (at most kTkLogBlocks blocks per launch).
static size_t tk_log_bytes(int64_t n_q, int32_t k, int32_t top) {
  if (n_q <= 0 || !topk_logs(top)) return 0;
  const int rg = topk_split_rg(k, top, true, n_q);
  const int64_t rows = 16 * (int64_t)tk_nw(kTopQ) * rg;  // query rows per block
  const int64_t blocks = std::min<int64_t>((n_q + rows - 1) / rows, kTkLogBlocks);
  const int topr = top <= 32 ? 32 : (top <= 64 ? 64 : (top <= 100 ? 100 : kTopQ));
  return align_up(sizeof(uint64_t) * (size_t)(blocks * rows) *
                  (size_t)tk_log_cap(topk_kq(k) / 32, topr));
}

size_t als_topk_workspace_bytes(int64_t n_q, int64_t n_v, int32_t k, int32_t top) {
  // 256 B of scale words | split planes of V in sweep order (2 x KQ halves per row) |
  // sweep order (int32 per V row) | bucket counts / cursors | scaled row norms in
  // sweep order (fp32 per V row) | 16 < top <= 128: per-row key logs
  return 256 + tk_table_bytes(n_v, k) + 2 * align_up(4 * (size_t)(n_v > 0 ? n_v : 0)) +
         align_up(4 * (size_t)kTkBuckets) + tk_log_bytes(n_q, k, top);
}

// als_topk (flt null) and als_topk_filtered share the argument checks, the workspace
// and V's preparation; only the sweep kernel differs.
static int topk_run(const float* Q, int64_t n_q, const float* V, int64_t n_v, int32_t ld,
                    int32_t k, int32_t top, int32_t* idx_out, float* score_out, void* ws,
                    size_t ws_bytes, void* stream, const RowFilter* flt) {
  ALS_REQUIRE(k >= 1 && k <= 128, ALS_EUNSUPPORTED, "als_topk: rank %d not in [1, 128]", k);
  ALS_REQUIRE(ld >= k && ld % 4 == 0, ALS_EINVAL, "als_topk: bad ld");
  ALS_REQUIRE(top >= 1 && top <= kTopkMax, ALS_EUNSUPPORTED, "als_topk: top %d not in [1, %d]",
              top, kTopkMax);
  ALS_REQUIRE(n_q >= 0 && n_v >= 0 && n_v < (int64_t(1) << 31), ALS_EINVAL,
              "als_topk: bad sizes");
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(Q && V && idx_out && score_out, ALS_EINVAL, "als_topk: null pointer");
  hipStream_t st = as_stream(stream);
  const bool logs = topk_logs(top);
  const int rg = topk_split_rg(k, top, logs, n_q);
  ALS_REQUIRE(rg > 0, ALS_EUNSUPPORTED, "als_topk: top %d at rank %d does not fit the LDS", top,
              k);
  ALS_REQUIRE(ws != nullptr && ws_bytes >= als_topk_workspace_bytes(n_q, n_v, k, top),
              ALS_EWORKSPACE, "als_topk: workspace %zu < %zu", ws_bytes,
              als_topk_workspace_bytes(n_q, n_v, k, top));
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_topk: workspace must be 16-byte aligned");
  unsigned* scal_u = static_cast<unsigned*>(ws);
  const float* scal = reinterpret_cast<const float*>(scal_u);
  _Float16* vsp = reinterpret_cast<_Float16*>(static_cast<char*>(ws) + 256);
  int32_t* perm = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + 256 + tk_table_bytes(n_v, k));
  int32_t* hist = perm + align_up(4 * (size_t)n_v) / 4;
  float* vnorm = reinterpret_cast<float*>(hist + align_up(4 * (size_t)kTkBuckets) / 4);
  uint64_t* tlog = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(vnorm) +
                                               align_up(4 * (size_t)(n_v > 0 ? n_v : 0)));
  const int kq = topk_kq(k);
  const int kq_shift = __builtin_ctz(kq);
  ALS_HIP(hipMemsetAsync(scal_u, 0, 2 * sizeof(unsigned), st));
  const int64_t nq_el = n_q * (int64_t)ld, nv_el = n_v * (int64_t)ld;
  tk_absmax_kernel<<<(int)std::min<int64_t>(256, (nq_el / 4 + 255) / 256 + 1), 256, 0, st>>>(
      Q, nq_el, scal_u);
  ALS_LAUNCH_CHECK();
  if (n_v > 0) {
    tk_absmax_kernel<<<(int)std::min<int64_t>(256, (nv_el / 4 + 255) / 256 + 1), 256, 0, st>>>(
        V, nv_el, scal_u + 1);
    ALS_LAUNCH_CHECK();
    // sweep order: V rows by decreasing norm (bucketed)
    ALS_HIP(hipMemsetAsync(hist, 0, sizeof(int32_t) * kTkBuckets, st));
    const int gb = (int)std::min<int64_t>(512, (n_v * 16 + 255) / 256);
    tk_bucket_hist_kernel<<<gb, 256, 0, st>>>(V, n_v, ld, k, scal, hist);
    ALS_LAUNCH_CHECK();
    tk_bucket_scan_kernel<<<1, 1024, 0, st>>>(hist);
    ALS_LAUNCH_CHECK();
    tk_bucket_scatter_kernel<<<gb, 256, 0, st>>>(V, n_v, ld, k, scal, hist, perm);
    ALS_LAUNCH_CHECK();
    const int64_t total = n_v << kq_shift;
    topk_split_table_kernel<<<(int)std::min<int64_t>(4096, (total + 255) / 256), 256, 0, st>>>(
        V, n_v, ld, k, kq_shift, scal, perm, vsp);
    ALS_LAUNCH_CHECK();
    tk_table_norm_kernel<<<(int)std::min<int64_t>(4096, (n_v * 16 + 255) / 256), 256, 0, st>>>(
        V, n_v, ld, k, scal, perm, vnorm);
    ALS_LAUNCH_CHECK();
  }
  const uint4* vsp4 = reinterpret_cast<const uint4*>(vsp);
  const TkLaunch a{Q, n_q, vsp4, vsp4 + n_v * (kq / 8), perm, vnorm, n_v, ld, k, top, scal,
                   idx_out, score_out, tlog, topk_split_lds_bytes(kq, rg, top, logs),
                   topk_nw(top, logs), rg, kq, logs, st};
  return flt ? topk_launch_filtered(a, *flt) : topk_launch_split(a, NoFilter{});
}

int als_topk(const float* Q, int64_t n_q, const float* V, int64_t n_v, int32_t ld, int32_t k,
             int32_t top, int32_t* idx_out, float* score_out, void* ws, size_t ws_bytes,
             void* stream) {
  return topk_run(Q, n_q, V, n_v, ld, k, top, idx_out, score_out, ws, ws_bytes, stream, nullptr);
}

int als_topk_filtered(const float* Q, int64_t n_q, const float* V, int64_t n_v, int32_t ld,
                      int32_t k, int32_t top, const int64_t* ex_begin, const int64_t* ex_end,
                      const int32_t* ex_col, const uint32_t* allow_bits, int32_t* idx_out,
                      float* score_out, void* ws, size_t ws_bytes, void* stream) {
  const int rc = check_exclusion_args("als_topk_filtered", ex_begin, ex_end, ex_col);
  if (rc != ALS_OK) return rc;
  const RowFilter flt{ex_begin, ex_end, ex_col, allow_bits};
  // no filter at all: the unfiltered kernel
  return topk_run(Q, n_q, V, n_v, ld, k, top, idx_out, score_out, ws, ws_bytes, stream,
                  (ex_begin || allow_bits) ? &flt : nullptr);
}

}  // extern "C"
