// K19 — co-rated neighbours: which rows of one side were rated together with this one, and
// how strongly.  The item-based collaborative-filtering neighbourhood (Sarwar et al. 2001;
// Linden et al. 2003), from the ratings themselves and not from the factors: one row of the
// sparse product B^T B per query, never formed.  Contract: include/als_hip.h.
//
// Take the item side: queries are items, B is the user x item multiplicity matrix.  Queries
// go through in passes of P; each query in flight owns a strip of n int32 counters.
//
// Plan (cr_plan_kernel, one wavefront).  Query row a of n_a entries is cut into
// ceil(n_a / task) tasks; the running task count per query (task_off) is all the later
// launches need, so no row length ever comes to the host.
// Count (cr_count_kernel).  A fixed grid of two workgroups per compute unit; the tasks are
// dealt to them in contiguous runs, so the tasks of the most-rated query are spread over
// the device and a workgroup rarely changes query.  For each entry (user u) of its task a
// wavefront walks u's row of the other block with coalesced col loads and adds 1 to the
// query's strip per entry, through the direct-mapped LDS cache of lx_cache.h (LDS add on a
// hit, one global add on a miss); the cache belongs to (workgroup, query) and is flushed
// and emptied when the workgroup moves to another query, and at its end.  Only integer
// adds: the strip holds c(a, .) exactly whatever order they land in.
// Rank (cr_rank_kernel).  One wavefront per (slice of the table, query): 64 counters and
// row lengths per step, self / min_common / candidates applied, the fp64 measure rounded
// once to fp32 and packed with the row into rank_key; the slice's `top` best survive in
// the log-and-cut of sim_lists.h.  The slice writes its keys and, beside each, the counter
// of that row, and then stores zeros over the strip slice it has read: the strips are
// zero again when the pass ends.
// Merge (sim_merge_kernel, two stages past 64 slices) orders the lists; cr_common_kernel
// finds each listed row's counter beside its key in the list of the row's slice.
#include "als_common.h"
#include "lx_cache.h"
#include "rank_key.h"
#include "sim_lists.h"

#include <algorithm>
#include <math.h>

namespace als {
namespace {

constexpr int kCrTask = 256;        // entries of a query row per task
constexpr int kCrTaskMax = 1 << 20;
constexpr int kCrPass = 32;         // queries per pass (pass = 0)
constexpr int kCrPassMax = 64;      // one lane per query in cr_plan_kernel
constexpr int kCrThreads = 512;     // count kernel: 8 wavefronts, 64 KiB of LDS
constexpr int kCrSliceRows = 2 * kSimTopMax;  // fewest rows of a slice, whatever `top`
constexpr int kCrMeasures = 3;      // 0 count, 1 jaccard, 2 cosine

// Entries of dense row `row` of a CSR side; 0 for a row outside [0, n).
__device__ __forceinline__ int64_t cr_row_len(const int64_t* __restrict__ row_ptr, int64_t n,
                                              int32_t row) {
  return (row >= 0 && row < n) ? row_ptr[row + 1] - row_ptr[row] : 0;
}

// task_off[q] = tasks of the pass's queries before q; task_off[nq] = all of them.
__global__ __launch_bounds__(64) void cr_plan_kernel(const int64_t* __restrict__ row_ptr_q,
                                                     int64_t n,
                                                     const int32_t* __restrict__ q_rows, int nq,
                                                     int task, int64_t* __restrict__ task_off) {
  const int lane = threadIdx.x & 63;
  const int64_t len = lane < nq ? cr_row_len(row_ptr_q, n, q_rows[lane]) : 0;
  int64_t incl = (len + task - 1) / task;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t up = shfl_up_64(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane < nq) task_off[lane + 1] = incl;
  if (lane == 0) task_off[0] = 0;
}

__global__ __launch_bounds__(kCrThreads) void cr_count_kernel(
    const int64_t* __restrict__ row_ptr_q, const int32_t* __restrict__ col_q, int64_t n,
    const int64_t* __restrict__ row_ptr_o, const int32_t* __restrict__ col_o, int64_t n_o,
    const int32_t* __restrict__ q_rows, int nq, int task, const int64_t* __restrict__ task_off,
    int32_t* __restrict__ strips) {
  __shared__ int32_t scnt[kLxWindow];
  __shared__ int32_t stag[kLxWindow];
  const int64_t total = task_off[nq];
  const int64_t per = (total + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * per;
  const int64_t t1 = t0 + per < total ? t0 + per : total;
  if (t0 >= t1) return;  // (the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lx_clear<kCrThreads>(scnt, stag);
  __syncthreads();
  int cur = -1;  // the query the cache holds counts of
  for (int64_t t = t0; t < t1; ++t) {
    int q = cur < 0 ? 0 : cur;  // the last query with task_off[q] <= t: the same in every thread
    while (q + 1 < nq && task_off[q + 1] <= t) ++q;
    if (q != cur) {
      if (cur >= 0) {
        __syncthreads();
        lx_flush<kCrThreads>(scnt, stag, strips + (int64_t)cur * n);
        __syncthreads();
        lx_clear<kCrThreads>(scnt, stag);
        __syncthreads();
      }
      cur = q;
    }
    int32_t* __restrict__ strip = strips + (int64_t)q * n;
    const int32_t row = q_rows[q];  // (a query with tasks has a row inside the table)
    const int64_t end = row_ptr_q[row + 1];
    const int64_t e0 = row_ptr_q[row] + (t - task_off[q]) * task;
    const int64_t e1 = e0 + task < end ? e0 + task : end;
    for (int64_t e = e0 + wave; e < e1; e += kCrThreads / 64) {
      const int32_t u = col_q[e];
      if ((uint32_t)u >= (uint64_t)n_o) continue;  // not a row of the other side: no walk
      const int64_t ue = row_ptr_o[u + 1];
      for (int64_t p = row_ptr_o[u] + lane; p < ue; p += 64) {
        const int32_t j = col_o[p];
        if ((uint32_t)j < (uint64_t)n) lx_add(j, scnt, stag, strip);
      }
    }
  }
  __syncthreads();
  lx_flush<kCrThreads>(scnt, stag, strips + (int64_t)cur * n);
}

// One measure of a pair: an fp64 expression of the three integers, rounded once to fp32.
__device__ __forceinline__ float cr_score(int measure, int32_t c, int64_t n_a, int64_t n_b) {
  if (measure == 0) return (float)c;
  if (measure == 1) return (float)((double)c / (double)(n_a + n_b - (int64_t)c));
  return (float)((double)c / sqrt((double)n_a * (double)n_b));
}

__global__ __launch_bounds__(64) void cr_rank_kernel(
    int32_t* __restrict__ strips, int64_t n, const int64_t* __restrict__ row_ptr_q,
    const int32_t* __restrict__ q_rows, int measure, int min_common,
    const uint32_t* __restrict__ allow, int top, int64_t rows_per_slice, int slices,
    uint64_t* __restrict__ keys_out, int32_t* __restrict__ common_out) {
  constexpr int JC = (sim_cap(kSimTopMax) + 63) / 64;
  __shared__ uint64_t lg[sim_cap(kSimTopMax)];
  const int lane = threadIdx.x & 63;
  const int slice = blockIdx.x, q = blockIdx.y;
  const int cap = sim_cap(top);
  const int32_t row_a = q_rows[q];
  const int64_t n_a = cr_row_len(row_ptr_q, n, row_a);
  int32_t* __restrict__ strip = strips + (int64_t)q * n;
  const int64_t r0 = std::min<int64_t>(n, slice * rows_per_slice);
  const int64_t r1 = std::min<int64_t>(n, r0 + rows_per_slice);
  int cnt = 0;
  uint64_t thr = 0;
  if (n_a > 0) {  // (an unknown or empty query lists nothing; its strip is zero)
    for (int64_t base = r0; base < r1; base += 64) {
      if (cnt + 64 > cap) {  // the next step could overflow the log: cut it to its `top` best
        thr = sim_compact<JC>(lg, cnt, top);
        cnt = top;
      }
      const int64_t b = base + lane;
      const int32_t c = b < r1 ? strip[b] : 0;
      bool pass = c >= min_common && b != row_a &&
                  (!allow || ((allow[b >> 5] >> (b & 31)) & 1u));
      uint64_t key = 0;
      if (pass) {
        key = rank_key(cr_score(measure, c, n_a, row_ptr_q[b + 1] - row_ptr_q[b]), (int)b);
        pass = key > thr;
      }
      const uint64_t m = __ballot(pass);
      if (pass) lg[cnt + __popcll(m & ((1ull << lane) - 1))] = key;
      cnt += __popcll(m);
      __syncthreads();
    }
    if (cnt > top) {
      sim_compact<JC>(lg, cnt, top);
      cnt = top;
    }
  }
  // the slice's `top` keys (unordered; open slots 0) and the counter of each, plain stores
  const int64_t o = ((int64_t)q * slices + slice) * top;
  for (int e = lane; e < top; e += 64) {
    const uint64_t key = e < cnt ? lg[e] : 0ull;
    keys_out[o + e] = key;
    common_out[o + e] = e < cnt ? strip[rank_key_index(key)] : 0;
  }
  __syncthreads();  // the counters above are read before the zeros below are stored
  for (int64_t b = r0 + lane; b < r1; b += 64) strip[b] = 0;
}

// common[q][t] of the ranked lists: the counter stored beside the key of row idx[q][t] in
// the list of that row's slice (every listed row is in its own slice's list).
__global__ __launch_bounds__(64) void cr_common_kernel(
    const int32_t* __restrict__ idx, int top, int64_t rows_per_slice, int slices,
    const uint64_t* __restrict__ keys, const int32_t* __restrict__ slice_common,
    int32_t* __restrict__ common) {
  const int q = blockIdx.x;
  for (int t = threadIdx.x; t < top; t += 64) {
    const int32_t j = idx[(int64_t)q * top + t];
    int32_t c = 0;
    if (j >= 0) {
      const int64_t s = j / rows_per_slice;
      if (s < slices) {
        const int64_t o = ((int64_t)q * slices + s) * top;
        for (int e = 0; e < top; ++e) {
          const uint64_t key = keys[o + e];
          if (key != 0ull && rank_key_index(key) == j) c = slice_common[o + e];
        }
      }
    }
    common[(int64_t)q * top + t] = c;
  }
}

// Slices of a table of n rows: 8 per compute unit, each of at least kCrSliceRows rows.
int cr_slices(int64_t n) {
  return (int)std::max<int64_t>(
      1, std::min<int64_t>(8 * (int64_t)sim_device_cus(), n / kCrSliceRows));
}

struct CrLayout {
  size_t strips, task_off, keys, slice_common, keys2, total;
  int pass, slices, groups;
};
// pass: the queries of one pass (the `pass` argument or kCrPass, at most n_q).
CrLayout cr_layout(int64_t n, int32_t n_q, int32_t top, int32_t pass) {
  CrLayout l;
  l.pass = std::max(1, std::min<int32_t>(n_q, pass > 0 ? pass : kCrPass));
  l.slices = cr_slices(n);
  l.groups = sim_groups(l.slices);
  const size_t lists = (size_t)l.pass * l.slices * top;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += align_up(bytes);
    return at;
  };
  l.strips = take(sizeof(int32_t) * (size_t)l.pass * (size_t)n);
  l.task_off = take(sizeof(int64_t) * (kCrPassMax + 1));
  l.keys = take(sizeof(uint64_t) * lists);
  l.slice_common = take(sizeof(int32_t) * lists);
  l.keys2 = take(sizeof(uint64_t) * (size_t)l.pass * l.groups * top);
  l.total = off;
  return l;
}

bool cr_sizes_ok(int64_t n, int32_t n_q, int32_t top, int32_t pass) {
  return n >= 0 && n < 2147483647ll && n_q >= 0 && top >= 1 && top <= kSimTopMax && pass >= 0 &&
         pass <= kCrPassMax;
}

}  // namespace
}  // namespace als

using namespace als;

extern "C" {

int32_t als_co_rated_task(void) { return kCrTask; }

int32_t als_co_rated_window(void) { return kLxWindow; }

size_t als_co_rated_scratch_bytes(int64_t n, int32_t n_q, int32_t top, int32_t pass) {
  if (!cr_sizes_ok(n, n_q, top, pass)) return 0;
  return cr_layout(n, n_q, top, pass).total;
}

int als_co_rated(const int64_t* row_ptr_q, const int32_t* col_q, int64_t n,
                 const int64_t* row_ptr_o, const int32_t* col_o, int64_t n_o,
                 const int32_t* q_rows, int32_t n_q, int32_t measure, int32_t min_common,
                 const uint32_t* allow_bits, int32_t top, int32_t pass, int32_t task,
                 int32_t* idx, float* score, int32_t* common, void* ws, size_t ws_bytes,
                 void* stream) {
  ALS_REQUIRE(top >= 1 && top <= kSimTopMax, ALS_EINVAL, "als_co_rated: top %d not in [1, %d]",
              top, kSimTopMax);
  ALS_REQUIRE(measure >= 0 && measure < kCrMeasures, ALS_EINVAL,
              "als_co_rated: measure %d not in [0, %d)", measure, kCrMeasures);
  ALS_REQUIRE(min_common >= 1, ALS_EINVAL, "als_co_rated: min_common %d < 1", min_common);
  ALS_REQUIRE(n >= 0 && n < 2147483647ll && n_o >= 0 && n_o < 2147483647ll && n_q >= 0,
              ALS_EINVAL, "als_co_rated: bad sizes");
  ALS_REQUIRE(pass >= 0 && pass <= kCrPassMax, ALS_EINVAL, "als_co_rated: pass %d not in [0, %d]",
              pass, kCrPassMax);
  ALS_REQUIRE(task >= 0 && task <= kCrTaskMax, ALS_EINVAL, "als_co_rated: task %d not in [0, %d]",
              task, kCrTaskMax);
  if (n_q == 0) return ALS_OK;
  ALS_REQUIRE(q_rows && idx && score && common, ALS_EINVAL, "als_co_rated: null pointer");
  ALS_REQUIRE(row_ptr_q && row_ptr_o, ALS_EINVAL, "als_co_rated: null row pointer");
  // (col_q / col_o may be null for a side without entries: no row then has any to read)
  const CrLayout l = cr_layout(n, n_q, top, pass);
  ALS_REQUIRE(ws != nullptr && ws_bytes >= l.total, ALS_EWORKSPACE,
              "als_co_rated: scratch %zu < %zu", ws_bytes, l.total);
  ALS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, ALS_EINVAL,
              "als_co_rated: scratch must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(ws);
  int32_t* strips = reinterpret_cast<int32_t*>(base + l.strips);
  int64_t* task_off = reinterpret_cast<int64_t*>(base + l.task_off);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + l.keys);
  int32_t* slice_common = reinterpret_cast<int32_t*>(base + l.slice_common);
  uint64_t* keys2 = reinterpret_cast<uint64_t*>(base + l.keys2);
  const int s = l.slices, groups = l.groups;
  const int64_t rows_per_slice = std::max<int64_t>(1, (n + s - 1) / s);
  const int tk = task > 0 ? task : kCrTask;
  const unsigned count_grid = 2u * (unsigned)sim_device_cus();
  // the strips start from zero whatever the scratch held; every pass leaves them zero
  if (n > 0)
    ALS_HIP(hipMemsetAsync(strips, 0, sizeof(int32_t) * (size_t)l.pass * (size_t)n, st));
  for (int32_t q0 = 0; q0 < n_q; q0 += l.pass) {
    const int nq = std::min<int32_t>(l.pass, n_q - q0);
    const int32_t* qp = q_rows + q0;
    cr_plan_kernel<<<1, 64, 0, st>>>(row_ptr_q, n, qp, nq, tk, task_off);
    ALS_LAUNCH_CHECK();
    cr_count_kernel<<<count_grid, kCrThreads, 0, st>>>(row_ptr_q, col_q, n, row_ptr_o, col_o, n_o,
                                                        qp, nq, tk, task_off, strips);
    ALS_LAUNCH_CHECK();
    cr_rank_kernel<<<dim3(s, nq), 64, 0, st>>>(strips, n, row_ptr_q, qp, measure, min_common,
                                               allow_bits, top, rows_per_slice, s, keys,
                                               slice_common);
    ALS_LAUNCH_CHECK();
    int32_t* io = idx + (int64_t)q0 * top;
    float* so = score + (int64_t)q0 * top;
    if (groups) {
      sim_merge_kernel<<<dim3(nq, groups), 64, 0, st>>>(keys, s, kSimMergeFan, top, keys2, nullptr,
                                                        nullptr, 0);
      ALS_LAUNCH_CHECK();
      sim_merge_kernel<<<dim3(nq, 1), 64, 0, st>>>(keys2, groups, groups, top, nullptr, io, so, 1);
    } else {
      sim_merge_kernel<<<dim3(nq, 1), 64, 0, st>>>(keys, s, s, top, nullptr, io, so, 1);
    }
    ALS_LAUNCH_CHECK();
    cr_common_kernel<<<nq, 64, 0, st>>>(io, top, rows_per_slice, s, keys, slice_common,
                                        common + (int64_t)q0 * top);
    ALS_LAUNCH_CHECK();
  }
  return ALS_OK;
}

}  // extern "C"
