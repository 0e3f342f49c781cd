// K5 — what the top-k sweep (topk_sweep.h) does with a score once it has one: the ranking
// rule, the filter's verdict on a refined block and the all-zero query rows under a filter,
// the sorted lists in LDS (top > 128), the register list's insertion (top <= 16) and the
// selection from a key log (16 < top <= 128).
#pragma once
#include "rank_key.h"
#include "topk_split.h"

namespace als {

constexpr int kTopkMax = 256;

__device__ __forceinline__ bool beats(float s1, int i1, float s2, int i2) {
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

// An all-zero query row under a filter: every score is 0, so its list is the first `top`
// admissible V rows by index (the unfiltered rule restricted to them), the rest open.
// One wave scans 64 V rows per step.
__device__ __forceinline__ void tk_zero_row_filtered(const RowFilter& f, int64_t row, int64_t n_v,
                                                     int top, int32_t* __restrict__ idx_out,
                                                     float* __restrict__ score_out) {
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  for (int64_t base = 0; base < n_v && cnt < top; base += 64) {
    const int64_t j = base + lane;
    const bool ok = j < n_v && row_admits(f, row, (int)j);
    const uint64_t b = __ballot(ok);
    const int pos = cnt + __popcll(b & ((1ull << lane) - 1));
    if (ok && pos < top) {
      idx_out[row * top + pos] = (int32_t)j;
      score_out[row * top + pos] = 0.f;
    }
    cnt += __popcll(b);
  }
  for (int e = (cnt < top ? cnt : top) + lane; e < top; e += 64) {
    idx_out[row * top + e] = -1;
    score_out[row * top + e] = -__builtin_inff();
  }
}

// The all-zero query rows among a wave's 16 RG rows (row0 + gr g + rho; live[g] bit rho
// clear and the row present; live is wave-uniform).
template <int RG>
__device__ __forceinline__ void tk_zero_rows_filtered(const RowFilter& f, const unsigned (&live)[RG],
                                                      int64_t row0, int gr, int64_t n_q,
                                                      int64_t n_v, int top,
                                                      int32_t* __restrict__ idx_out,
                                                      float* __restrict__ score_out) {
#pragma unroll
  for (int g = 0; g < RG; ++g)
    for (int rho = 0; rho < 16; ++rho) {
      const int64_t row = row0 + gr * g + rho;
      if (row < n_q && !((live[g] >> rho) & 1u))
        tk_zero_row_filtered(f, row, n_v, top, idx_out, score_out);
    }
}

// A refined 16 x 16 block per row group (acc[g][r] = exact score of query row
// row0 + gr g + r, r = 0..3 of this lane's quarter, against V row j): the pairs that would
// go on to a list or log (score at or above th[g][r]; all: every pair, while lists are
// still filling) and are inadmissible score NaN from here on.  Dead rows (absent: no
// exclusion range to read; or all zero) likewise.
template <int RG, class TH>
__device__ __forceinline__ void tk_drop_inadmissible(const RowFilter& f, floatx4 (&acc)[RG], int j,
                                                     const TH& th, bool all,
                                                     const unsigned (&live)[RG], int64_t row0,
                                                     int gr) {
  const int q = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int g = 0; g < RG; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // the verdict as a flag and one select after the branch (with `acc[g][r] = NaN`
      // assigned inside the branch, the gfx950 code hipcc 7 generated restored the
      // score for every lane that ran the test: seen in the assembly, and as excluded
      // rows listed on the device)
      bool drop = false;
      if (acc[g][r] == acc[g][r] && (all || acc[g][r] >= th[g][r])) {
        const bool lv = (live[g] >> (4 * q + r)) & 1u;
        drop = !lv || !row_admits(f, row0 + gr * g + r, j);
      }
      acc[g][r] = drop ? __builtin_nanf("") : acc[g][r];
    }
}

// Offer one 16 x 16 score block to the sorted per-row lists (64-bit keys, best
// first): acc[r] = score of list row slot0 + 4q + r against V row ibase + m.
// Candidates that beat their row's current k-th (score, index) are inserted one at
// a time by the whole wave (rank by ballot, shift, insert), lowest lane first.  The
// rank is counted from the tail: past the fill, a new key usually lands in the last
// 64 entries, so one LDS pass finds it.
__device__ __forceinline__ void topk_offer(const floatx4& acc, int ibase, int64_t n_v,
                                           const int32_t* __restrict__ bperm, float (&ts)[4],
                                           int (&ti)[4], uint64_t* __restrict__ lk,
                                           int* __restrict__ len, int slot0, int top,
                                           unsigned live) {
  const int lane = threadIdx.x & 63, q = lane >> 4;
  const int m = lane & 15;
  const bool vin = (int64_t)(ibase + m) < n_v;
  // V row index of table row ibase + m (the sweep is norm-ordered; bperm = the
  // block's slice of the tile's order in LDS)
  const int vidx = vin ? bperm[m] : 0x7fffffff;
  int pend = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (vin && ((live >> (4 * q + r)) & 1u) && beats(acc[r], vidx, ts[r], ti[r])) pend |= 1 << r;
  uint64_t any = __ballot(pend != 0);
  while (any) {
    const int L = __builtin_ctzll(any);
    const int myr = pend ? __builtin_ctz(pend) : 0;
    const float mys = myr == 0 ? acc[0] : (myr == 1 ? acc[1] : (myr == 2 ? acc[2] : acc[3]));
    const int rL = __builtin_amdgcn_readlane(myr, L);
    const float sc =
        __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mys), L));
    const int itm = __builtin_amdgcn_readlane(vidx, L);
    const uint64_t ck = rank_key(sc, itm);
    const int slot = slot0 + 4 * (L >> 4) + rL;  // list row within the workgroup
    uint64_t* lkr = lk + slot * top;
    const int n = len[slot];
    // pos = number of entries that beat the candidate = n - (entries it beats);
    // scan 64-entry windows from the tail until one holds an entry that beats it
    int worse = 0;
    for (int e1 = n; e1 > 0; e1 -= 64) {
      const int e = e1 - 64 + lane;
      const int cnt = __popcll(__ballot(e >= 0 && lkr[e < 0 ? 0 : e] < ck));
      worse += cnt;
      if (cnt < (e1 < 64 ? e1 : 64)) break;
    }
    const int pos = n - worse;
    if (pos < top) {
      const int newn = n + 1 < top ? n + 1 : top;
      uint64_t hk[kTopkMax / 64];
#pragma unroll
      for (int j = 0; j < kTopkMax / 64; ++j) {
        const int e = 64 * j + lane;
        if (e > pos && e < newn) hk[j] = lkr[e - 1];
      }
      // reads of the shifted entries land before any lane writes (compiler + HW order)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int j = 0; j < kTopkMax / 64; ++j) {
        const int e = 64 * j + lane;
        if (e > pos && e < newn) lkr[e] = hk[j];
      }
      if (lane == 0) {
        lkr[pos] = ck;
        len[slot] = newn;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (newn == top) {
        const uint64_t kk = lkr[top - 1];
        const float ks = rank_key_score(kk);
        const int ki = rank_key_index(kk);
        if (q == (L >> 4)) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r == rL) {
              ts[r] = ks;
              ti[r] = ki;
            }
        }
      }
    }
    if (lane == L) pend &= ~(1 << rL);
    // drop pending candidates of that row that no longer beat its threshold
    if (q == (L >> 4)) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r == rL && (pend >> r & 1) && !beats(acc[r], vidx, ts[r], ti[r])) pend &= ~(1 << r);
    }
    any = __ballot(pend != 0);
  }
}

// Write the lists of rows slot0 .. slot0+15 (one wave) to the outputs.
__device__ __forceinline__ void topk_write(const uint64_t* __restrict__ lk,
                                           const int* __restrict__ len, int slot0, int64_t qbase,
                                           int64_t n_q, int64_t n_v, int top, float unscale,
                                           unsigned live, int32_t* __restrict__ idx_out,
                                           float* __restrict__ score_out,
                                           bool zero_rows = true) {
  const int lane = threadIdx.x & 63;
  for (int rr = 0; rr < 16; ++rr) {
    const int slot = slot0 + rr;
    const int64_t row = qbase + slot;
    if (row >= n_q) break;
    if (!((live >> rr) & 1u)) {  // all-zero query row: every score is 0, ties by index
      if (!zero_rows) continue;  // (filtered: tk_zero_row_filtered writes them)
      for (int e = lane; e < top; e += 64) {
        idx_out[row * top + e] = e < n_v ? e : -1;
        score_out[row * top + e] = e < n_v ? 0.f : -__builtin_inff();
      }
      continue;
    }
    const int n = len[slot];
    for (int e = lane; e < top; e += 64) {
      const uint64_t kk = e < n ? lk[slot * top + e] : 0ull;
      idx_out[row * top + e] = e < n ? rank_key_index(kk) : -1;
      score_out[row * top + e] = e < n ? rank_key_score(kk) * unscale : -__builtin_inff();
    }
  }
}

// Insert key `c` into a list sorted ascending (the k-th best at [0]; sentinels past
// `top`).  c_j = c > key_j is monotone (true for j < p); the list becomes
// [.. keys 1..p-1, c, keys p..]: independent selects, no chain.  The caller has
// checked c > [0].
template <int TOPR>
__device__ __forceinline__ void tk_insert(uint64_t (&kv)[TOPR], uint64_t c) {
  bool gt[TOPR + 1];
#pragma unroll
  for (int j = 0; j < TOPR; ++j) gt[j] = c > kv[j];
  gt[TOPR] = false;
#pragma unroll
  for (int j = 0; j < TOPR; ++j) {
    const uint64_t nx = j + 1 < TOPR ? kv[j + 1] : 0ull;
    kv[j] = gt[j + 1] ? nx : (gt[j] ? c : kv[j]);
  }
}

// The T-th largest of the n keys of log L (n <= 64 J, 1 <= T <= n): the largest P
// with #{keys >= P} >= T.  Keys are unique ((score, V row) pairs), so exactly T keys are
// >= P.  The wave's lanes hold the keys (kv[j] = L[64 j + lane], 0 past n: below every
// real key).  A bitwise search over the 32 score bits first (the T-th largest score S);
// when the keys scoring S are exactly the ones still needed, P is the least of them (a
// min over the wave); only with more ties at S than needed does a second bitwise search
// over the index bits of those keys run.
template <int J>
__device__ __forceinline__ uint64_t tk_log_kth(const uint64_t (&kv)[J], int T) {
  uint32_t S = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t cand = S | (1u << b);
    int c = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) c += __popcll(__ballot((uint32_t)(kv[j] >> 32) >= cand));
    if (c >= T) S = cand;
  }
  int gt = 0, eq = 0;
  uint32_t lmin = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const uint32_t h = (uint32_t)(kv[j] >> 32);
    gt += __popcll(__ballot(h > S));
    eq += __popcll(__ballot(h == S));
    if (h == S) lmin = min(lmin, (uint32_t)kv[j]);
  }
  const int need = T - gt;  // 1 <= need <= eq
  if (need == eq) {  // every key scoring S is kept: P is the least of them
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lmin = min(lmin, (uint32_t)__shfl_xor((int)lmin, o));
    return ((uint64_t)S << 32) | lmin;
  }
  uint32_t L = 0;  // the need-th largest index word among the keys scoring S
  for (int b = 31; b >= 0; --b) {
    const uint32_t cand = L | (1u << b);
    int c = 0;
#pragma unroll
    for (int j = 0; j < J; ++j)
      c += __popcll(__ballot((uint32_t)(kv[j] >> 32) == S && (uint32_t)kv[j] >= cand));
    if (c >= need) L = cand;
  }
  return ((uint64_t)S << 32) | L;
}

}  // namespace als
