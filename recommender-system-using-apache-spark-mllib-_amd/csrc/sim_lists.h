// The list machinery of the slice-and-merge neighbour searches, shared by the cosine
// neighbours (K12, similar.hip) and the co-rated neighbours (K19, co_rated.hip): the cut of a
// log of 64-bit rank keys to its `top` largest (sim_compact), the merge of per-slice lists
// (sim_merge_kernel) and the slice / merge-group counts of a call.  Each including file gets
// its own copy (anonymous namespace), as it had when similar.hip held them alone.
#pragma once
#include "als_common.h"
#include "rank_key.h"

#include <algorithm>

namespace als {
namespace {

constexpr int kSimTopMax = 256;
constexpr int kSimMergeCap = 512;  // keys of the merge kernel's log
constexpr int kSimMaxSlices = 4096;
constexpr int kSimMergeFan = 32;   // slice lists per first-stage merge group

// Cut log L (n keys, top < n <= 64 J, unique, all > 0; one wavefront, L in LDS) to its `top`
// largest keys, in place at the front; returns the smallest kept key.  The top-th largest
// score word first (bitwise search, the method of topk_lists.h's tk_log_kth), then the index
// word among the keys that tie on it.
template <int J>
__device__ __forceinline__ uint64_t sim_compact(uint64_t* __restrict__ L, int n, int top) {
  const int lane = threadIdx.x & 63;
  uint64_t kv[J];
#pragma unroll
  for (int j = 0; j < J; ++j) kv[j] = 64 * j + lane < n ? L[64 * j + lane] : 0ull;
  uint32_t S = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t cand = S | (1u << b);
    int c = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) c += __popcll(__ballot((uint32_t)(kv[j] >> 32) >= cand));
    if (c >= top) S = cand;
  }
  int gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t h = (uint32_t)(kv[j] >> 32);
    gt += __popcll(__ballot(h > S));
    eq += __popcll(__ballot(h == S));
  }
  const int need = top - gt;  // 1 <= need <= eq
  uint32_t Lw = 0;            // the need-th largest index word among the keys scoring S
  if (need < eq) {
    for (int b = 31; b >= 0; --b) {
      const uint32_t cand = Lw | (1u << b);
      int c = 0;
#pragma unroll
      for (int j = 0; j < J; ++j)
        c += __popcll(__ballot((uint32_t)(kv[j] >> 32) == S && (uint32_t)kv[j] >= cand));
      if (c >= need) Lw = cand;
    }
  }
  const uint64_t P = ((uint64_t)S << 32) | Lw;  // need == eq: every key scoring S is kept
  int base = 0;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const bool kp = kv[j] >= P && kv[j] != 0ull;
    const uint64_t b = __ballot(kp);
    if (kp) L[base + __popcll(b & ((1ull << lane) - 1))] = kv[j];
    base += __popcll(b);
  }
  __syncthreads();  // (one wavefront: orders the LDS writes before the reads that follow)
  uint64_t lo = ~0ull;  // the smallest kept key (P itself, or the least key scoring S)
#pragma unroll
  for (int j = 0; j < J; ++j)
    if (kv[j] >= P && kv[j] != 0ull) lo = kv[j] < lo ? kv[j] : lo;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t a = (uint32_t)__shfl_xor((int)(uint32_t)lo, o);
    const uint32_t bb = (uint32_t)__shfl_xor((int)(uint32_t)(lo >> 32), o);
    const uint64_t other = ((uint64_t)bb << 32) | a;
    lo = other < lo ? other : lo;
  }
  return lo;
}

__host__ __device__ constexpr int sim_cap(int top) { return (top + 64 + 63) / 64 * 64; }

// lists x top keys of query blockIdx.x (in + (query lists + first list) top ...) -> the
// `top` largest: as keys for a later stage (final = 0: out_keys[(query groups + group) top
// ..], unordered, open slots 0) or ranked and unpacked (final = 1).
__global__ __launch_bounds__(64) void sim_merge_kernel(const uint64_t* __restrict__ in, int lists,
                                                       int per_group, int top,
                                                       uint64_t* __restrict__ out_keys,
                                                       int32_t* __restrict__ idx_out,
                                                       float* __restrict__ score_out, int final) {
  __shared__ uint64_t L[kSimMergeCap];
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x, g = blockIdx.y, groups = gridDim.y;
  const int l0 = g * per_group, l1 = std::min(lists, l0 + per_group);
  const uint64_t* p = in + ((int64_t)j * lists + l0) * top;
  const int64_t m = (int64_t)(l1 - l0) * top;
  int cnt = 0;
  uint64_t thr = 0;
  for (int64_t i = 0; i < m; i += 64) {
    if (cnt + 64 > kSimMergeCap) {
      thr = sim_compact<kSimMergeCap / 64>(L, cnt, top);
      cnt = top;
    }
    const uint64_t key = i + lane < m ? p[i + lane] : 0ull;
    const bool pass = key > thr;
    const uint64_t b = __ballot(pass);
    if (pass) L[cnt + __popcll(b & ((1ull << lane) - 1))] = key;
    cnt += __popcll(b);
    __syncthreads();
  }
  if (cnt > top) {
    sim_compact<kSimMergeCap / 64>(L, cnt, top);
    cnt = top;
  }
  if (!final) {
    uint64_t* o = out_keys + ((int64_t)j * groups + g) * top;
    for (int e = lane; e < top; e += 64) o[e] = e < cnt ? L[e] : 0ull;
    return;
  }
  for (int e = lane; e < top; e += 64) {
    if (e < cnt) {
      const uint64_t key = L[e];
      int rank = 0;  // keys are unique: the rank is the number of larger keys
      for (int i = 0; i < cnt; ++i) rank += L[i] > key;
      idx_out[(int64_t)j * top + rank] = rank_key_index(key);
      score_out[(int64_t)j * top + rank] = rank_key_score(key);
    } else {
      idx_out[(int64_t)j * top + e] = -1;
      score_out[(int64_t)j * top + e] = -__builtin_inff();
    }
  }
}

// Compute units of the current device; 256 (an MI355X) where no device answers, so that the
// size functions run on a host without one.
int sim_device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        v > 0)
      cus = v;
    else
      cus = 256;  // (sizing without a device: an MI355X)
  }
  return cus;
}

// Slices of a call: `slices` as given, or (0) 8 per compute unit, capped so that a slice
// holds at least max(256, 2 top) rows.
int sim_slices(int64_t n, int top, int slices) {
  if (slices > 0) return slices;
  const int cus = sim_device_cus();
  const int64_t min_rows = std::max<int64_t>(256, 2 * (int64_t)top);
  return (int)std::max<int64_t>(1, std::min<int64_t>(8 * (int64_t)cus, n / min_rows));
}

int sim_groups(int slices) {
  return slices > 64 ? (slices + kSimMergeFan - 1) / kSimMergeFan : 0;
}

}  // namespace
}  // namespace als
