// K15 — what the lists of all users look like together: item exposure counts, their
// concentration (coverage, Gini, entropy, pair overlap) and the popularity of what is listed
// (novelty, average popularity, long-tail share).
//
// Replaces nothing in Spark.  The measures are the usual beyond-accuracy ones: catalogue
// coverage (Herlocker et al. 2004), novelty as mean self-information and personalisation as
// one minus the mean overlap of two lists (Zhou et al. 2010), average recommendation
// popularity and the long-tail share (Abdollahpouri et al.).  Contracts: include/als_hip.h.
//
// als_list_exposure is a histogram of up to 1e9 Zipf-skewed keys over up to 1e6 bins.  Each
// workgroup keeps kLxWindow int32 counters in LDS, used as a direct-mapped cache of the
// catalogue: key j lives in slot j mod kLxWindow, the first key to reach a slot claims it
// (one LDS compare-and-swap on the slot's tag), and from then on every entry naming that key
// is one LDS integer add.  A key that finds its slot taken by another goes to memory with one
// global integer add.  When the workgroup has run out of lists it adds every non-zero slot to
// counts[] once.  A catalogue of at most kLxWindow rows therefore never collides (the cache
// is a plain privatised window), and in a larger, skewed one the rows that take most of the
// entries are the ones most likely to arrive first and own their slots.  Every add is an
// integer add, so counts are exact and the same bits whatever order the adds land in.
//
// als_list_concentration and als_list_novelty sum in fp64 in a fixed order (partial_sums.h).
#include "als_common.h"
#include "lx_cache.h"
#include "partial_sums.h"
#include <math.h>

namespace als {

constexpr int kLmMaxAt = 256;

// An entry counts when it names a row of the catalogue: 0 <= j < n_v, and bit j of allow
// (als_topk_filtered's mask; NULL: every row).
__device__ __forceinline__ bool list_entry_valid(int32_t j, int32_t n_v,
                                                 const uint32_t* __restrict__ allow) {
  if ((uint32_t)j >= (uint32_t)n_v) return false;
  return !allow || ((allow[j >> 5] >> (j & 31)) & 1u);
}

// ---------------------------------------------------------------------------------------
// als_list_exposure
// ---------------------------------------------------------------------------------------
// (the cache itself, kLxWindow slots claimed and added to by lx_add: lx_cache.h)
constexpr int kLxThreads = 1024;
constexpr int kLxMaxBlocks = 512;      // two workgroups per compute unit
constexpr int kLxChunkEntries = 16384; // list slots a workgroup takes at a time

// Rows go through in chunks of rows_per_chunk (rows_per_chunk * at < 2^31, so a slot's row and
// position come from one 32-bit division); workgroups stride over the chunks.
__global__ __launch_bounds__(kLxThreads) void list_exposure_kernel(
    const int32_t* __restrict__ idx, int64_t n_q, int idx_ld, int at, int32_t n_v,
    const uint32_t* __restrict__ allow, int rows_per_chunk, int32_t* __restrict__ counts,
    unsigned long long* __restrict__ n_skipped) {
  __shared__ int32_t scnt[kLxWindow];
  __shared__ int32_t stag[kLxWindow];
  __shared__ unsigned long long sskip;
  lx_clear<kLxThreads>(scnt, stag);
  if (threadIdx.x == 0) sskip = 0ull;
  __syncthreads();
  unsigned long long skipped = 0ull;
  const int64_t n_chunks = (n_q + rows_per_chunk - 1) / rows_per_chunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t r0 = c * rows_per_chunk;
    const int64_t left = n_q - r0;
    const uint32_t nr = left < rows_per_chunk ? (uint32_t)left : (uint32_t)rows_per_chunk;
    const uint32_t ne = nr * (uint32_t)at;
    for (uint32_t i = threadIdx.x; i < ne; i += kLxThreads) {
      const uint32_t lr = i / (uint32_t)at, p = i - lr * (uint32_t)at;
      const int32_t j = idx[(r0 + lr) * (int64_t)idx_ld + p];
      if (list_entry_valid(j, n_v, allow)) lx_add(j, scnt, stag, counts);
      else ++skipped;
    }
  }
  if (skipped) atomicAdd(&sskip, skipped);
  __syncthreads();
  lx_flush<kLxThreads>(scnt, stag, counts);
  if (threadIdx.x == 0 && n_skipped && sskip) atomicAdd(n_skipped, sskip);
}

// ---------------------------------------------------------------------------------------
// als_list_concentration
// ---------------------------------------------------------------------------------------
constexpr int kLcMaxBlocks = 1024;
constexpr int kLcFieldsA = 4;  // catalogue rows, rows listed, total, pair overlap
constexpr int kLcFieldsB = 2;  // Gini numerator, entropy

static inline int64_t lc_blocks(int64_t n_v) {
  const int64_t g = (n_v + 2047) / 2048;
  return g < 1 ? 1 : (g > kLcMaxBlocks ? kLcMaxBlocks : g);
}

// Row order: the sort key of every row (its count inside the catalogue, 0 outside) and the
// integer-valued sums.  Thread t of block b takes rows b*256 + t, + 256*gridDim.x, ...
__global__ __launch_bounds__(256) void lc_keys_kernel(const int32_t* __restrict__ counts,
                                                      int64_t n_v,
                                                      const uint32_t* __restrict__ allow,
                                                      uint32_t* __restrict__ keys,
                                                      int32_t* __restrict__ vals,
                                                      double* __restrict__ partial) {
  __shared__ double sm[256];
  double a_n = 0.0, a_cov = 0.0, a_tot = 0.0, a_pair = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_v; j += 256ll * gridDim.x) {
    const bool in = list_entry_valid((int32_t)j, (int32_t)n_v, allow);
    const int32_t c = in ? counts[j] : 0;
    const uint32_t key = c > 0 ? (uint32_t)c : 0u;
    keys[j] = key;
    vals[j] = (int32_t)j;
    if (in) a_n += 1.0;
    if (key) {
      const double cd = (double)key;
      a_cov += 1.0;
      a_tot += cd;
      a_pair += cd * (cd - 1.0) * 0.5;
    }
  }
  const double v[kLcFieldsA] = {a_n, a_cov, a_tot, a_pair};
  for (int f = 0; f < kLcFieldsA; ++f) {
    const double s = block_tree_sum(v[f], sm);
    if (threadIdx.x == 0) partial[(int64_t)kLcFieldsA * blockIdx.x + f] = s;
  }
}

// Sorted order: position i of the ascending keys holds the count of catalogue rank
// i + 1 - (n_v - n); the rows outside the catalogue and the unlisted ones are the leading
// zeros and add nothing.
__global__ __launch_bounds__(256) void lc_sorted_kernel(const uint32_t* __restrict__ skeys,
                                                        int64_t n_v,
                                                        const double* __restrict__ tot_a,
                                                        double* __restrict__ partial) {
  __shared__ double sm[256];
  const double n = tot_a[0], total = tot_a[2];
  const double lead = (double)n_v - n;
  double a_g = 0.0, a_h = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_v; i += 256ll * gridDim.x) {
    const uint32_t key = skeys[i];
    if (key) {
      const double c = (double)key;
      const double rank = (double)(i + 1) - lead;
      a_g += (2.0 * rank - n - 1.0) * c;
      const double p = c / total;
      a_h -= p * log2(p);
    }
  }
  const double v[kLcFieldsB] = {a_g, a_h};
  for (int f = 0; f < kLcFieldsB; ++f) {
    const double s = block_tree_sum(v[f], sm);
    if (threadIdx.x == 0) partial[(int64_t)kLcFieldsB * blockIdx.x + f] = s;
  }
}

__global__ void lc_finish_kernel(const double* __restrict__ tot_a, const double* __restrict__ tot_b,
                                 const uint32_t* __restrict__ skeys, int64_t n_v,
                                 double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double n = tot_a[0], total = tot_a[2];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  out[0] = n;
  out[1] = tot_a[1];
  out[2] = total;
  out[3] = total > 0.0 ? tot_b[0] / (n * total) : nan;
  out[4] = total > 0.0 ? tot_b[1] : nan;
  out[5] = tot_a[3];
  out[6] = (double)skeys[n_v - 1];
}

__global__ void lc_empty_kernel(double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  out[0] = out[1] = out[2] = out[5] = out[6] = 0.0;
  out[3] = out[4] = nan;
}

struct LcLayout {
  size_t keys, vals, skeys, svals, part_a, part_b, tot, sort, total;
};
static LcLayout lc_layout(int64_t n_v) {
  LcLayout l;
  const size_t n = n_v > 0 ? (size_t)n_v : 1, nb = (size_t)lc_blocks(n_v);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += align_up(bytes);
    return at;
  };
  l.keys = take(sizeof(uint32_t) * n);
  l.vals = take(sizeof(int32_t) * n);
  l.skeys = take(sizeof(uint32_t) * n);
  l.svals = take(sizeof(int32_t) * n);
  l.part_a = take(sizeof(double) * kLcFieldsA * nb);
  l.part_b = take(sizeof(double) * kLcFieldsB * nb);
  l.tot = take(sizeof(double) * (kLcFieldsA + kLcFieldsB));
  l.sort = take(radix_workspace_bytes((int64_t)n));
  l.total = off;
  return l;
}

// ---------------------------------------------------------------------------------------
// als_list_novelty
// ---------------------------------------------------------------------------------------
constexpr int kLnRowsPerBlock = 4;   // one wavefront each
constexpr int kLnMaxBlocks = 4096;   // blocks stride over the row groups past this
constexpr int kLnSums = 7;

static inline int64_t ln_blocks(int64_t n_q) {
  const int64_t g = (n_q + kLnRowsPerBlock - 1) / kLnRowsPerBlock;
  return g < 1 ? 1 : (g > kLnMaxBlocks ? kLnMaxBlocks : g);
}

__device__ __forceinline__ double shfl_f64(double v, int lane) {
  int2 iv = __builtin_bit_cast(int2, v);
  iv.x = __shfl(iv.x, lane);
  iv.y = __shfl(iv.y, lane);
  return __builtin_bit_cast(double, iv);
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    int2 iv = __builtin_bit_cast(int2, v);
    iv.x = __shfl_xor(iv.x, m);
    iv.y = __shfl_xor(iv.y, m);
    v += __builtin_bit_cast(long long, iv);
  }
  return v;
}

// One wavefront per list (the structure of rank_metrics_kernel).  Lane l takes positions l,
// l + 64, ...; the self-information terms of a pass are added by walking the ballot mask, so
// a row's fp64 sum runs in position order; the popularity sum and the two counts are
// integers.  Every lane of a wave carries the same sums.
__global__ __launch_bounds__(256) void list_novelty_kernel(
    const int32_t* __restrict__ idx, int64_t n_q, int idx_ld, int at, int32_t n_v,
    const uint32_t* __restrict__ allow, const int32_t* __restrict__ pop, double n_pop,
    const uint32_t* __restrict__ tail, double* __restrict__ per_row,
    double* __restrict__ partial) {
  __shared__ double swave[kLnRowsPerBlock][kLnSums];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double s_nov = 0.0, s_nov_rows = 0.0, s_arp = 0.0, s_rows = 0.0, s_tail = 0.0, s_valid = 0.0,
         s_skip = 0.0;
  const int64_t n_grp = (n_q + kLnRowsPerBlock - 1) / kLnRowsPerBlock;
  for (int64_t g = blockIdx.x; g < n_grp; g += gridDim.x) {
    const int64_t r = g * kLnRowsPerBlock + w;
    if (r >= n_q) continue;  // wave-uniform; no barrier inside the loop
    const int32_t* __restrict__ row = idx + r * (int64_t)idx_ld;
    double nov = 0.0;
    int n_nov = 0, n_valid = 0, n_tail = 0;
    long long pop_sum = 0;
    for (int p0 = 0; p0 < at; p0 += 64) {
      const int p = p0 + lane;
      const int32_t j = p < at ? row[p] : -1;
      const bool ok = list_entry_valid(j, n_v, allow);
      const int32_t pj = ok ? pop[j] : 0;
      const bool has = ok && pj > 0;
      const double term = has ? log2(n_pop / (double)pj) : 0.0;
      uint64_t mask = __ballot(has);
      n_nov += __popcll(mask);
      n_valid += __popcll(__ballot(ok));
      if (tail) n_tail += __popcll(__ballot(ok && ((tail[j >> 5] >> (j & 31)) & 1u)));
      pop_sum += wave_sum_i64((long long)pj);
      while (mask) {  // the pass's terms in position order
        const int q = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        nov += shfl_f64(term, q);
      }
    }
    const double nov_r = n_nov > 0 ? nov / (double)n_nov : nan;
    const double arp_r = n_valid > 0 ? (double)pop_sum / (double)n_valid : nan;
    const double tail_r = (tail && n_valid > 0) ? (double)n_tail / (double)n_valid : nan;
    if (n_nov > 0) {
      s_nov += nov_r;
      s_nov_rows += 1.0;
    }
    if (n_valid > 0) {
      s_arp += arp_r;
      s_rows += 1.0;
      if (tail) s_tail += tail_r;
    }
    s_valid += (double)n_valid;
    s_skip += (double)(at - n_valid);
    if (per_row && lane == 0) {
      per_row[r * 3] = nov_r;
      per_row[r * 3 + 1] = arp_r;
      per_row[r * 3 + 2] = tail_r;
    }
  }
  if (lane == 0) {
    swave[w][0] = s_nov;
    swave[w][1] = s_nov_rows;
    swave[w][2] = s_arp;
    swave[w][3] = s_rows;
    swave[w][4] = s_tail;
    swave[w][5] = s_valid;
    swave[w][6] = s_skip;
  }
  __syncthreads();
  if (threadIdx.x < kLnSums) {
    double a = 0.0;
    for (int i = 0; i < kLnRowsPerBlock; ++i) a += swave[i][threadIdx.x];
    partial[(int64_t)kLnSums * blockIdx.x + threadIdx.x] = a;
  }
}

// The checks the three entry points share (the header's list).
static int check_lists(const char* who, int64_t n_q, int32_t idx_ld, int32_t at, int64_t n_v) {
  ALS_REQUIRE(at >= 1 && at <= kLmMaxAt, ALS_EUNSUPPORTED, "%s: at = %d outside [1, %d]", who,
              at, kLmMaxAt);
  ALS_REQUIRE(idx_ld >= at, ALS_EINVAL, "%s: idx_ld %d < at %d", who, idx_ld, at);
  ALS_REQUIRE(n_q >= 0, ALS_EINVAL, "%s: n_q < 0", who);
  ALS_REQUIRE(n_v >= 0 && n_v < 2147483647ll, ALS_EINVAL, "%s: n_v outside [0, 2^31 - 1)", who);
  return ALS_OK;
}

}  // namespace als

using namespace als;

extern "C" {

int32_t als_list_exposure_window(void) { return kLxWindow; }

int als_list_exposure(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at, int64_t n_v,
                      const uint32_t* allow_bits, int accumulate, int32_t* counts,
                      int64_t* n_skipped_dev, void* stream) {
  int rc = check_lists("als_list_exposure", n_q, idx_ld, at, n_v);
  if (rc) return rc;
  ALS_REQUIRE(counts || n_v == 0, ALS_EINVAL, "als_list_exposure: null counts");
  ALS_REQUIRE(idx || n_q == 0, ALS_EINVAL, "als_list_exposure: null idx");
  hipStream_t st = as_stream(stream);
  if (!accumulate) {
    if (n_v > 0) ALS_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_v, st));
    if (n_skipped_dev) ALS_HIP(hipMemsetAsync(n_skipped_dev, 0, sizeof(int64_t), st));
  }
  if (n_q == 0) return ALS_OK;
  int rows_per_chunk = kLxChunkEntries / at;
  if (rows_per_chunk < 1) rows_per_chunk = 1;
  const int64_t n_chunks = (n_q + rows_per_chunk - 1) / rows_per_chunk;
  const unsigned nb = (unsigned)(n_chunks > kLxMaxBlocks ? kLxMaxBlocks : n_chunks);
  unsigned long long* skip = reinterpret_cast<unsigned long long*>(n_skipped_dev);
  list_exposure_kernel<<<nb, kLxThreads, 0, st>>>(idx, n_q, idx_ld, at, (int32_t)n_v, allow_bits,
                                                   rows_per_chunk, counts, skip);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

size_t als_list_concentration_scratch_bytes(int64_t n_v) {
  if (n_v < 0 || n_v >= 2147483647ll) return 0;
  return lc_layout(n_v).total;
}

int als_list_concentration(const int32_t* counts, int64_t n_v, const uint32_t* allow_bits,
                           int64_t n_lists, int32_t at, double* out, void* ws, size_t ws_bytes,
                           void* stream) {
  ALS_REQUIRE(at >= 1 && at <= kLmMaxAt, ALS_EUNSUPPORTED,
              "als_list_concentration: at = %d outside [1, %d]", at, kLmMaxAt);
  ALS_REQUIRE(n_lists >= 0, ALS_EINVAL, "als_list_concentration: n_lists < 0");
  ALS_REQUIRE(n_v >= 0 && n_v < 2147483647ll, ALS_EINVAL,
              "als_list_concentration: n_v outside [0, 2^31 - 1)");
  ALS_REQUIRE(out, ALS_EINVAL, "als_list_concentration: null out");
  hipStream_t st = as_stream(stream);
  if (n_v == 0) {
    lc_empty_kernel<<<1, 64, 0, st>>>(out);
    ALS_LAUNCH_CHECK();
    return ALS_OK;
  }
  ALS_REQUIRE(counts, ALS_EINVAL, "als_list_concentration: null counts");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_list_concentration: workspace not 16-byte aligned");
  const LcLayout l = lc_layout(n_v);
  ALS_REQUIRE(ws && ws_bytes >= l.total, ALS_EWORKSPACE,
              "als_list_concentration: workspace too small");
  char* base = static_cast<char*>(ws);
  uint32_t* keys = reinterpret_cast<uint32_t*>(base + l.keys);
  int32_t* vals = reinterpret_cast<int32_t*>(base + l.vals);
  uint32_t* skeys = reinterpret_cast<uint32_t*>(base + l.skeys);
  int32_t* svals = reinterpret_cast<int32_t*>(base + l.svals);
  double* part_a = reinterpret_cast<double*>(base + l.part_a);
  double* part_b = reinterpret_cast<double*>(base + l.part_b);
  double* tot_a = reinterpret_cast<double*>(base + l.tot);
  double* tot_b = tot_a + kLcFieldsA;
  const int64_t nb = lc_blocks(n_v);
  lc_keys_kernel<<<(unsigned)nb, 256, 0, st>>>(counts, n_v, allow_bits, keys, vals, part_a);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kLcFieldsA><<<1, 256, 0, st>>>(part_a, nb, tot_a);
  ALS_LAUNCH_CHECK();
  // radix_sort_pairs carries a payload; nothing reads the sorted row indices (svals).  All 32
  // key bits are sorted: the largest count is not known on the host.
  int rc = radix_sort_pairs(keys, vals, skeys, svals, n_v, 32, base + l.sort,
                            l.total - l.sort, st);
  if (rc) return rc;
  lc_sorted_kernel<<<(unsigned)nb, 256, 0, st>>>(skeys, n_v, tot_a, part_b);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kLcFieldsB><<<1, 256, 0, st>>>(part_b, nb, tot_b);
  ALS_LAUNCH_CHECK();
  lc_finish_kernel<<<1, 64, 0, st>>>(tot_a, tot_b, skeys, n_v, out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

size_t als_list_novelty_scratch_bytes(int64_t n_q) {
  return align_up(sizeof(double) * kLnSums * (size_t)ln_blocks(n_q));
}

int als_list_novelty(const int32_t* idx, int64_t n_q, int32_t idx_ld, int32_t at, int64_t n_v,
                     const uint32_t* allow_bits, const int32_t* pop, int64_t n_pop,
                     const uint32_t* tail_bits, double* sums_out, double* per_row_out,
                     void* ws, size_t ws_bytes, void* stream) {
  int rc = check_lists("als_list_novelty", n_q, idx_ld, at, n_v);
  if (rc) return rc;
  ALS_REQUIRE(n_pop >= 1, ALS_EINVAL, "als_list_novelty: n_pop < 1");
  ALS_REQUIRE(sums_out, ALS_EINVAL, "als_list_novelty: null sums_out");
  hipStream_t st = as_stream(stream);
  if (n_q == 0) {
    ALS_HIP(hipMemsetAsync(sums_out, 0, kLnSums * sizeof(double), st));
    return ALS_OK;
  }
  ALS_REQUIRE(idx && (pop || n_v == 0), ALS_EINVAL, "als_list_novelty: null pointer");
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_list_novelty: workspace not 16-byte aligned");
  ALS_REQUIRE(ws && ws_bytes >= als_list_novelty_scratch_bytes(n_q), ALS_EWORKSPACE,
              "als_list_novelty: workspace too small");
  double* partial = static_cast<double*>(ws);
  const int64_t nb = ln_blocks(n_q);
  list_novelty_kernel<<<(unsigned)nb, 256, 0, st>>>(idx, n_q, idx_ld, at, (int32_t)n_v,
                                                    allow_bits, pop, (double)n_pop, tail_bits,
                                                    per_row_out, partial);
  ALS_LAUNCH_CHECK();
  sum_partials_kernel<kLnSums><<<1, 256, 0, st>>>(partial, nb, sums_out);
  ALS_LAUNCH_CHECK();
  return ALS_OK;
}

}  // extern "C"
