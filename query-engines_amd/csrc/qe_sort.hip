// ORDER BY (build-defined operator): stable multi-key sort to row indices, and
// the gather by row index that applies them.
//
// qe_sort_indices
//   Every key becomes bits of one long unsigned key (qe_sort_key.hpp), most significant key first;
//   the key is cut into 64-bit words, word 0 the least significant. LSD radix sort over
//   (word, int32 row index) pairs with 8-bit digits, words from the last to the first:
//     k_sort_encode : word k of every row, read through the current permutation, plus all 8 digit
//                     histograms of that word (one read-back per word: a digit that is constant
//                     over all rows costs no pass)
//     per executed digit:
//       k_sort_count   : digit counts per tile of SORT_TILE rows (digit-major)
//       exclusive scan : global start of every (digit, tile) run
//       k_sort_scatter : ranks the tile's rows (ballot match inside a wave, wave totals through
//                        LDS), stages the pairs in LDS in output order, writes each digit's rows
//                        as one contiguous run
//   n <= SORT_SMALL_MAX: k_sort_small, one workgroup, every word and digit in LDS, one launch.
// qe_topk_indices
//   The first k rows of the same stable order by radix selection from the most significant digit
//   down (host rules: qe_topk_plan.hpp): k_topk_words (digit histograms; the first pass writes
//   nothing else), per digit step k_topk_count / exclusive scan / k_topk_compact over a candidate
//   list kept in row order, then k_sort_small_rows or the passes above over the candidates.
// qe_take
//   k_take: one row per lane, validity / BOOL words built per wave with __ballot; UTF8 through the
//   (start, length) pairs, length scan and byte copy of qe_filter.hip.
// qe_take_or_null
//   k_take<true>: index -1 is "no row" and gives a null row (the build side of a LEFT join).
// sort_pairs
//   the count / scan / scatter passes over a caller's (word, index) buffers (qe_join.hip).
#include "qe_internal.hpp"
#include "qe_sort_key.hpp"
#include "qe_topk_plan.hpp"

namespace qe {

// Build-time shape of the multi-workgroup passes. Measured at 100M full-range INT64 rows (ms per
// sort): 256 x 16 11.5, 512 x 8 9.6, 1024 x 4 9.2 (same tile, more waves to hide the loads).
#ifndef QE_SORT_THREADS
#define QE_SORT_THREADS 1024
#endif
#ifndef QE_SORT_ITEMS
#define QE_SORT_ITEMS 4
#endif
constexpr int SORT_THREADS = QE_SORT_THREADS;
constexpr int SORT_ITEMS = QE_SORT_ITEMS;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS;  // 4096 rows: 48 KB of staged pairs
constexpr int SORT_SMALL_THREADS = 256;
constexpr int SORT_SMALL_ITEMS = 8;
constexpr int SORT_SMALL_MAX = SORT_SMALL_THREADS * SORT_SMALL_ITEMS;  // 2048 rows: two 24 KB pair buffers
static_assert(SORT_THREADS >= 256 && SORT_THREADS % 64 == 0 && SORT_TILE * 12 <= 48 * 1024, "sort tile shape");
constexpr int64_t SORT_MAX_WORDS = 4096;                        // a key of at most 32 KiB

enum { SK_FIXED = 0, SK_UTF8_SHORT = 1, SK_UTF8 = 2 };

struct SortKey {
  const void* values;
  const uint8_t* validity;
  const int32_t* offsets;
  int32_t type, flags;
  int32_t mode;     // SK_FIXED (fixed-width / BOOL), SK_UTF8_SHORT (7 bytes + length byte), SK_UTF8
  int32_t vbits;    // width of the value field: the type's bits; 64 (short UTF8); 32 (UTF8 byte length)
  int64_t lo_v;     // key bit of the value field's least significant bit
  int64_t lo_n;     // key bit of the null bit, -1: the column has no validity
  int64_t cw0;      // SK_UTF8: the 8-byte chunks are whole words cw0 .. cw0 + nchunks - 1, last chunk first
  int64_t nchunks;
};

struct SortDesc {
  SortKey key[QE_MAX_KEYS];
  int32_t nkeys;
  int32_t nwords;
};

// Big-endian bytes [8c, 8c + 8) of a value of `len` bytes at `p`, zero-padded.
__device__ __forceinline__ uint64_t utf8_chunk(const uint8_t* __restrict__ p, int32_t len, int64_t c) {
  uint64_t w = 0;
  const int64_t b0 = 8 * c;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w <<= 8;
    if (b0 + j < len) w |= p[b0 + j];
  }
  return w;
}

// Word k of row r's key. *err is set when a short UTF8 key's value exceeds its promised 7 bytes.
__device__ __forceinline__ uint64_t sort_word(const SortDesc& D, int64_t r, int64_t k, unsigned* err) {
  uint64_t w = 0;
  const int64_t b0 = 64 * k, b1 = b0 + 64;
  for (int q = 0; q < D.nkeys; ++q) {
    const SortKey& K = D.key[q];
    const bool in_v = K.lo_v < b1 && K.lo_v + K.vbits > b0;
    const bool in_n = K.lo_n >= b0 && K.lo_n < b1;
    const bool in_c = K.mode == SK_UTF8 && k >= K.cw0 && k < K.cw0 + K.nchunks;
    if (!(in_v || in_n || in_c)) continue;
    const bool valid = !K.validity || ((K.validity[r >> 3] >> (r & 7)) & 1);
    if (in_n) w |= sort_null_bit(valid, K.flags) << (K.lo_n - b0);
    if (!valid) continue;
    if (K.mode == SK_FIXED) {
      uint64_t raw;
      switch (K.type) {
        case QE_TYPE_INT64:
        case QE_TYPE_FLOAT64: raw = ((const uint64_t*)K.values)[r]; break;
        case QE_TYPE_INT32:
        case QE_TYPE_DATE32: raw = ((const uint32_t*)K.values)[r]; break;
        case QE_TYPE_UINT8: raw = ((const uint8_t*)K.values)[r]; break;
        default: raw = (((const uint8_t*)K.values)[r >> 3] >> (r & 7)) & 1; break;  // BOOL
      }
      w |= sort_place(sort_field(sort_enc_fixed(K.type, raw), K.vbits, true, K.flags), K.lo_v, k);
    } else {
      const int32_t s = K.offsets[r];
      int32_t len = K.offsets[r + 1] - s;
      if (len < 0) len = 0;
      const uint8_t* p = (const uint8_t*)K.values + s;
      if (K.mode == SK_UTF8_SHORT) {
        if (len > 7) {
          *err = 1u;
          len = 7;
        }
        const uint64_t asc = utf8_chunk(p, len, 0) | (uint64_t)len;  // 7 bytes, then the length byte
        w |= sort_place(sort_field(asc, 64, true, K.flags), K.lo_v, k);
      } else {
        if (in_v) w |= sort_place(sort_field((uint64_t)(uint32_t)len, 32, true, K.flags), K.lo_v, k);
        if (in_c) w |= sort_field(utf8_chunk(p, len, K.cw0 + K.nchunks - 1 - k), 64, true, K.flags);
      }
    }
  }
  return w;
}

// One more row with digit d in the LDS histogram h; a wave whose active lanes all hold the same
// digit (a constant or narrow-range key) adds once.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t d) {
  const uint64_t act = __ballot(1);
  const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
  if (__ballot(d == d0) == act) {
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(act)) atomicAdd(&h[d0], (uint32_t)__popcll(act));
  } else {
    atomicAdd(&h[d], 1u);
  }
}

__global__ void __launch_bounds__(256) k_utf8_max_len(const int32_t* __restrict__ offs, int64_t n,
                                                      int32_t* __restrict__ out) {
  int32_t mx = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    mx = max(mx, offs[i + 1] - offs[i]);
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
  if ((threadIdx.x & 63) == 0 && mx > 0) atomicMax(out, mx);
}

// words[i] = word k of row perm[i] (perm NULL: row i, and idx_out[i] = i); hist[256 g + v] += rows
// whose digit g of that word is v.
constexpr int ENC_THREADS = 256;
__global__ void __launch_bounds__(ENC_THREADS) k_sort_encode(SortDesc D, int64_t k, int64_t n,
                                                              const int32_t* __restrict__ perm,
                                                              uint64_t* __restrict__ words, int32_t* __restrict__ idx_out,
                                                              uint32_t* __restrict__ hist, unsigned* __restrict__ err) {
  __shared__ uint32_t h[8 * 256];
  for (int j = threadIdx.x; j < 8 * 256; j += ENC_THREADS) h[j] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)ENC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * ENC_THREADS) {
    int64_t r = perm ? (int64_t)perm[i] : i;
    if ((uint64_t)r >= (uint64_t)n) r = 0;  // (a permutation never is)
    const uint64_t w = sort_word(D, r, k, err);
    words[i] = w;
    if (idx_out) idx_out[i] = (int32_t)i;
#pragma unroll
    for (int g = 0; g < 8; ++g) hist_add(h + 256 * g, (uint32_t)(w >> (8 * g)) & 255u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 8 * 256; j += ENC_THREADS)
    if (h[j]) atomicAdd(&hist[j], h[j]);
}

// counts[d * ntiles + tile] = rows of the tile whose digit is d.
__global__ void __launch_bounds__(SORT_THREADS) k_sort_count(const uint64_t* __restrict__ words, int64_t n, int shift,
                                                             int64_t ntiles, int64_t* __restrict__ counts) {
  __shared__ uint32_t h[256];
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * SORT_TILE;
#pragma unroll 4
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const int64_t g = t0 + it * SORT_THREADS + threadIdx.x;
    if (g < n) hist_add(h, (uint32_t)(words[g] >> shift) & 255u);
  }
  __syncthreads();
  if (threadIdx.x < 256) counts[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// Stable positions of a workgroup's THREADS * ITEMS rows ordered by digit. Row p of the tile is item
// `it` of lane `lane` of wave `wid` with p = wid * 64 * ITEMS + it * 64 + lane, so every wave owns a
// contiguous run of rows and counts its digits alone. pos[it] = the row's position in the sorted
// tile; dstart[d] = position of the tile's first row with digit d.
template <int THREADS, int ITEMS>
__device__ __forceinline__ void tile_rank(const uint32_t (&dig)[ITEMS], uint32_t (&pos)[ITEMS],
                                          uint16_t (*wcnt)[256], uint32_t* dstart, uint32_t* wsum) {
  constexpr int WAVES = THREADS / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1;
  for (int j = threadIdx.x; j < WAVES * 256; j += THREADS) (&wcnt[0][0])[j] = 0;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const uint32_t d = dig[it];
    uint64_t m = ~0ull;  // lanes of this wave whose digit equals d
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const uint64_t bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const uint32_t r = (uint32_t)__popcll(m & lt);
    const uint32_t base = wcnt[wid][d];
    __builtin_amdgcn_wave_barrier();
    if (r == 0) wcnt[wid][d] = (uint16_t)(base + (uint32_t)__popcll(m));  // the digit's first lane counts its lanes
    __builtin_amdgcn_wave_barrier();
    pos[it] = base + r;
  }
  __syncthreads();
  uint32_t run = 0, x = 0;  // thread t < 256 (the first four waves): digit t over the waves
  if (threadIdx.x < 256) {
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t c = wcnt[w][threadIdx.x];
      wcnt[w][threadIdx.x] = (uint16_t)run;  // (a tile holds at most 4096 rows)
      run += c;
    }
    x = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t y = __shfl_up(x, off);
      if (lane >= off) x += y;
    }
    if (lane == 63) wsum[wid] = x;
  }
  __syncthreads();
  if (threadIdx.x < 256) {
    uint32_t wp = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) wp += w < wid ? wsum[w] : 0;
    dstart[threadIdx.x] = wp + x - run;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) pos[it] += dstart[dig[it]] + wcnt[wid][dig[it]];
}

// One stable pass of the tile: rows of [t0, t0 + SORT_TILE) go to offs[digit * ntiles + tile] + their
// rank among the tile's rows of that digit. wout NULL: the words are not needed again.
__global__ void __launch_bounds__(SORT_THREADS) k_sort_scatter(const uint64_t* __restrict__ win,
                                                               const int32_t* __restrict__ iin,
                                                               uint64_t* __restrict__ wout, int32_t* __restrict__ iout,
                                                               int64_t n, int shift, int64_t ntiles,
                                                               const int64_t* __restrict__ offs) {
  __shared__ uint64_t s_word[SORT_TILE];
  __shared__ int32_t s_idx[SORT_TILE];
  __shared__ uint16_t s_wcnt[SORT_THREADS / 64][256];
  __shared__ uint32_t s_dstart[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ int64_t s_delta[256];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * SORT_TILE;
  const int64_t m = min((int64_t)SORT_TILE, n - t0);
  uint64_t w[SORT_ITEMS];
  int32_t ix[SORT_ITEMS];
  uint32_t dig[SORT_ITEMS], pos[SORT_ITEMS];
#pragma unroll
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const int p = wid * (64 * SORT_ITEMS) + it * 64 + lane;
    const bool live = p < m;
    // rows past the end take digit 255: they are the last rows of the tile, so they rank last
    w[it] = live ? win[t0 + p] : ~0ull;
    ix[it] = live ? iin[t0 + p] : 0;
    dig[it] = live ? (uint32_t)(w[it] >> shift) & 255u : 255u;
  }
  tile_rank<SORT_THREADS, SORT_ITEMS>(dig, pos, s_wcnt, s_dstart, s_wsum);
#pragma unroll
  for (int it = 0; it < SORT_ITEMS; ++it) {
    if (pos[it] < (uint32_t)SORT_TILE) {
      s_word[pos[it]] = w[it];
      s_idx[pos[it]] = ix[it];
    }
  }
  if (threadIdx.x < 256)
    s_delta[threadIdx.x] = offs[(int64_t)threadIdx.x * ntiles + blockIdx.x] - (int64_t)s_dstart[threadIdx.x];
  __syncthreads();
#pragma unroll 4
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const int p = it * SORT_THREADS + threadIdx.x;
    if (p < m) {
      const uint64_t ww = s_word[p];
      const int64_t o = s_delta[(uint32_t)(ww >> shift) & 255u] + p;
      if ((uint64_t)o < (uint64_t)n) {
        if (wout) wout[o] = ww;
        iout[o] = s_idx[p];
      }
    }
  }
}

// n <= SORT_SMALL_MAX rows in one workgroup and one launch: for every word, encode through the
// current permutation, find the digits that vary (OR xor AND over the rows), and run their stable
// passes between two LDS pair buffers. out[0 .. m_out) = the first rows of the order.
__global__ void __launch_bounds__(SORT_SMALL_THREADS) k_sort_small(SortDesc D, int32_t n, int32_t m_out,
                                                             int32_t* __restrict__ out, unsigned* __restrict__ err) {
  __shared__ uint64_t s_word[2][SORT_SMALL_MAX];
  __shared__ int32_t s_idx[2][SORT_SMALL_MAX];
  constexpr int WAVES = SORT_SMALL_THREADS / 64;
  __shared__ uint16_t s_wcnt[WAVES][256];
  __shared__ uint32_t s_dstart[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ uint64_t s_or[WAVES], s_and[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int cur = 0;
  for (int p = threadIdx.x; p < n; p += SORT_SMALL_THREADS) s_idx[0][p] = p;
  __syncthreads();
  for (int k = 0; k < D.nwords; ++k) {
    uint64_t o = 0, a = ~0ull;
    for (int p = threadIdx.x; p < n; p += SORT_SMALL_THREADS) {
      int32_t r = s_idx[cur][p];
      if ((uint32_t)r >= (uint32_t)n) r = 0;
      const uint64_t w = sort_word(D, r, k, err);
      s_word[cur][p] = w;
      o |= w;
      a &= w;
    }
    for (int off = 32; off > 0; off >>= 1) {
      o |= __shfl_xor(o, off);
      a &= __shfl_xor(a, off);
    }
    if (lane == 0) {
      s_or[wid] = o;
      s_and[wid] = a;
    }
    __syncthreads();
    o = 0;
    a = ~0ull;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      o |= s_or[w];
      a &= s_and[w];
    }
    __syncthreads();
    const uint64_t diff = o ^ a;  // bits that are not the same in every row (the same in every thread)
    for (int g = 0; g < 8; ++g) {
      if (((diff >> (8 * g)) & 255u) == 0) continue;
      uint64_t w[SORT_SMALL_ITEMS];
      int32_t ix[SORT_SMALL_ITEMS];
      uint32_t dig[SORT_SMALL_ITEMS], pos[SORT_SMALL_ITEMS];
#pragma unroll
      for (int it = 0; it < SORT_SMALL_ITEMS; ++it) {
        const int p = wid * (64 * SORT_SMALL_ITEMS) + it * 64 + lane;
        const bool live = p < n;
        w[it] = live ? s_word[cur][p] : ~0ull;
        ix[it] = live ? s_idx[cur][p] : 0;
        dig[it] = live ? (uint32_t)(w[it] >> (8 * g)) & 255u : 255u;
      }
      tile_rank<SORT_SMALL_THREADS, SORT_SMALL_ITEMS>(dig, pos, s_wcnt, s_dstart, s_wsum);
#pragma unroll
      for (int it = 0; it < SORT_SMALL_ITEMS; ++it) {
        if (pos[it] < (uint32_t)SORT_SMALL_MAX) {
          s_word[cur ^ 1][pos[it]] = w[it];
          s_idx[cur ^ 1][pos[it]] = ix[it];
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  for (int p = threadIdx.x; p < m_out; p += SORT_SMALL_THREADS) out[p] = s_idx[cur][p];
}

// k_sort_small over a row list (the top-k's final sort): the rows are the n entries of `rows` (row
// indices below nrows, flag bit 31 ignored), not 0 .. n - 1, and rows that compare equal keep the
// list's order. A kernel of its own, so that k_sort_small stays the kernel it was.
__global__ void __launch_bounds__(SORT_SMALL_THREADS) k_sort_small_rows(SortDesc D, int32_t n, int32_t nrows,
                                                                  const int32_t* __restrict__ rows, int32_t m_out,
                                                                  int32_t* __restrict__ out, unsigned* __restrict__ err) {
  __shared__ uint64_t s_word[2][SORT_SMALL_MAX];
  __shared__ int32_t s_idx[2][SORT_SMALL_MAX];
  constexpr int WAVES = SORT_SMALL_THREADS / 64;
  __shared__ uint16_t s_wcnt[WAVES][256];
  __shared__ uint32_t s_dstart[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ uint64_t s_or[WAVES], s_and[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int cur = 0;
  for (int p = threadIdx.x; p < n; p += SORT_SMALL_THREADS) s_idx[0][p] = rows[p] & 0x7FFFFFFF;
  __syncthreads();
  for (int k = 0; k < D.nwords; ++k) {
    uint64_t o = 0, a = ~0ull;
    for (int p = threadIdx.x; p < n; p += SORT_SMALL_THREADS) {
      int32_t r = s_idx[cur][p];
      if ((uint32_t)r >= (uint32_t)nrows) r = 0;
      const uint64_t w = sort_word(D, r, k, err);
      s_word[cur][p] = w;
      o |= w;
      a &= w;
    }
    for (int off = 32; off > 0; off >>= 1) {
      o |= __shfl_xor(o, off);
      a &= __shfl_xor(a, off);
    }
    if (lane == 0) {
      s_or[wid] = o;
      s_and[wid] = a;
    }
    __syncthreads();
    o = 0;
    a = ~0ull;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      o |= s_or[w];
      a &= s_and[w];
    }
    __syncthreads();
    const uint64_t diff = o ^ a;  // bits that are not the same in every row (the same in every thread)
    for (int g = 0; g < 8; ++g) {
      if (((diff >> (8 * g)) & 255u) == 0) continue;
      uint64_t w[SORT_SMALL_ITEMS];
      int32_t ix[SORT_SMALL_ITEMS];
      uint32_t dig[SORT_SMALL_ITEMS], pos[SORT_SMALL_ITEMS];
#pragma unroll
      for (int it = 0; it < SORT_SMALL_ITEMS; ++it) {
        const int p = wid * (64 * SORT_SMALL_ITEMS) + it * 64 + lane;
        const bool live = p < n;
        w[it] = live ? s_word[cur][p] : ~0ull;
        ix[it] = live ? s_idx[cur][p] : 0;
        dig[it] = live ? (uint32_t)(w[it] >> (8 * g)) & 255u : 255u;
      }
      tile_rank<SORT_SMALL_THREADS, SORT_SMALL_ITEMS>(dig, pos, s_wcnt, s_dstart, s_wsum);
#pragma unroll
      for (int it = 0; it < SORT_SMALL_ITEMS; ++it) {
        if (pos[it] < (uint32_t)SORT_SMALL_MAX) {
          s_word[cur ^ 1][pos[it]] = w[it];
          s_idx[cur ^ 1][pos[it]] = ix[it];
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  }
  for (int p = threadIdx.x; p < m_out; p += SORT_SMALL_THREADS) out[p] = s_idx[cur][p];
}

// ---- top-k: radix selection (qe_topk_plan.hpp holds the host's rules) ------------------------------
// The candidate list: row indices in ascending row order, bit 31 set on a sure row. A tied row's
// current key word lies beside it; a sure row's word is never read again. Before the first
// compaction the list is implicit: every row, all tied.
constexpr uint32_t TOPK_SURE = 0x80000000u;
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_ITEMS = 16;
constexpr int TOPK_TILE = TOPK_THREADS * TOPK_ITEMS;  // candidates per workgroup of a compaction
static_assert(TOPK_TILE == SORT_TILE, "qe_sort_layout reports one tile size");

// Key words of list entries, and the 8 digit histograms of the rows it encodes.
//   TW_ALL  : the implicit list, rows 0 .. m - 1; nothing but the histograms is written
//   TW_TIED : word k of the tied entries of `cand` -> words[i]
//   TW_SORT : word k of every entry of `cand` -> words[i]; `strip`: the flag bits leave `cand` (the
//             final sort's first word: from here on the list is the sort's permutation)
enum { TW_ALL = 0, TW_TIED = 1, TW_SORT = 2 };
template <int MODE>
__global__ void __launch_bounds__(ENC_THREADS) k_topk_words(SortDesc D, int64_t k, int64_t nrows, int64_t m,
                                                             int32_t* __restrict__ cand, uint64_t* __restrict__ words,
                                                             int strip, uint32_t* __restrict__ hist,
                                                             unsigned* __restrict__ err) {
  __shared__ uint32_t h[8 * 256];
  for (int j = threadIdx.x; j < 8 * 256; j += ENC_THREADS) h[j] = 0;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)ENC_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * ENC_THREADS) {
    int64_t r = i;
    if (MODE != TW_ALL) {
      const uint32_t c = (uint32_t)cand[i];
      if (MODE == TW_TIED && (c & TOPK_SURE)) continue;
      r = (int64_t)(c & ~TOPK_SURE);
      if (MODE == TW_SORT && strip) cand[i] = (int32_t)r;
    }
    if ((uint64_t)r >= (uint64_t)nrows) r = 0;  // (a candidate never is)
    const uint64_t w = sort_word(D, r, k, err);
    if (MODE != TW_ALL) words[i] = w;
#pragma unroll
    for (int g = 0; g < 8; ++g) hist_add(h + 256 * g, (uint32_t)(w >> (8 * g)) & 255u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 8 * 256; j += ENC_THREADS)
    if (h[j]) atomicAdd(&hist[j], h[j]);
}

struct TopkStep {
  int64_t k;         // the key word in play
  int32_t shift;     // 8 x its digit in play
  uint32_t bin;      // the threshold bin: a tied row with a smaller digit becomes sure, a larger one leaves
  int32_t cut_only;  // no digit is in play: every tied row stays tied (the cut after the last digit)
  int32_t pad;
  int64_t cut;       // the tied rows that stay: the first `cut` in row order
};

// What becomes of candidate i under step S: 0 it leaves, 1 sure, 2 tied. *w = its word when tied before.
template <bool ALL>
__device__ __forceinline__ uint32_t topk_class(const SortDesc& D, const TopkStep& S, int64_t i,
                                               const int32_t* __restrict__ cand, const uint64_t* __restrict__ words,
                                               int32_t* row, uint64_t* w, unsigned* err) {
  if (ALL) {
    *row = (int32_t)i;
    *w = sort_word(D, i, S.k, err);
  } else {
    const uint32_t c = (uint32_t)cand[i];
    *row = (int32_t)(c & ~TOPK_SURE);
    if (c & TOPK_SURE) return 1u;
    *w = words[i];
  }
  if (S.cut_only) return 2u;
  const uint32_t d = (uint32_t)(*w >> S.shift) & 255u;
  return d < S.bin ? 1u : d == S.bin ? 2u : 0u;
}

// counts[tile] = candidates of the tile that stay as sure rows, counts[ntiles + tile] = as tied rows
// (before the cut).
template <bool ALL>
__global__ void __launch_bounds__(TOPK_THREADS) k_topk_count(SortDesc D, TopkStep S, int64_t m,
                                                              const int32_t* __restrict__ cand,
                                                              const uint64_t* __restrict__ words, int64_t ntiles,
                                                              int64_t* __restrict__ counts, unsigned* __restrict__ err) {
  __shared__ uint32_t s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * TOPK_TILE;
  uint32_t ns = 0, nt = 0;
  for (int it = 0; it < TOPK_ITEMS; ++it) {
    const int64_t i = t0 + it * TOPK_THREADS + threadIdx.x;
    uint32_t cls = 0;
    if (i < m) {
      int32_t row;
      uint64_t w = 0;
      cls = topk_class<ALL>(D, S, i, cand, words, &row, &w, err);
    }
    ns += (uint32_t)__popcll(__ballot(cls == 1u));
    nt += (uint32_t)__popcll(__ballot(cls == 2u));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&s_cnt[0], ns);
    atomicAdd(&s_cnt[1], nt);
  }
  __syncthreads();
  if (threadIdx.x < 2) counts[(int64_t)threadIdx.x * ntiles + blockIdx.x] = s_cnt[threadIdx.x];
}

// The stable compaction of one tile. Candidate p of the tile is item `it` of lane `lane` of wave
// `wid` with p = wid * 64 * ITEMS + it * 64 + lane, so a wave owns a contiguous run and ranks it by
// ballots alone. offs = the exclusive scan of k_topk_count's counts: a staying row goes to
// (sure rows before it) + min(tied rows before it, cut), and a tied row stays iff fewer than `cut`
// tied rows precede it, which keeps the list in ascending row order. hist (may be NULL): the 8 digit
// histograms of the rows that stay tied, for the next step's pick.
template <bool ALL>
__global__ void __launch_bounds__(TOPK_THREADS) k_topk_compact(SortDesc D, TopkStep S, int64_t m,
                                                                const int32_t* __restrict__ cand,
                                                                const uint64_t* __restrict__ words, int64_t ntiles,
                                                                const int64_t* __restrict__ offs, int64_t mout,
                                                                int32_t* __restrict__ cand_out,
                                                                uint64_t* __restrict__ words_out,
                                                                uint32_t* __restrict__ hist, unsigned* __restrict__ err) {
  constexpr int WAVES = TOPK_THREADS / 64;
  __shared__ uint32_t h[8 * 256];
  __shared__ uint32_t s_ws[WAVES], s_wt[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1;
  if (hist)
    for (int j = threadIdx.x; j < 8 * 256; j += TOPK_THREADS) h[j] = 0;
  const int64_t t0 = (int64_t)blockIdx.x * TOPK_TILE + wid * (64 * TOPK_ITEMS);
  uint64_t w[TOPK_ITEMS];
  int32_t row[TOPK_ITEMS];
  uint32_t cls = 0, ns = 0, nt = 0;  // 2 class bits per item; this wave's totals
#pragma unroll
  for (int it = 0; it < TOPK_ITEMS; ++it) {
    const int64_t i = t0 + it * 64 + lane;
    uint32_t c = 0;
    w[it] = 0;
    row[it] = 0;
    if (i < m) c = topk_class<ALL>(D, S, i, cand, words, &row[it], &w[it], err);
    cls |= c << (2 * it);
    ns += (uint32_t)__popcll(__ballot(c == 1u));
    nt += (uint32_t)__popcll(__ballot(c == 2u));
  }
  if (lane == 0) {
    s_ws[wid] = ns;
    s_wt[wid] = nt;
  }
  __syncthreads();
  // rows that stay before this wave's first: the earlier tiles' (from the scan) and the earlier waves'
  int64_t sb = offs[blockIdx.x], tb = offs[ntiles + blockIdx.x] - offs[ntiles];
#pragma unroll
  for (int v = 0; v < WAVES; ++v) {
    if (v < wid) {
      sb += s_ws[v];
      tb += s_wt[v];
    }
  }
#pragma unroll
  for (int it = 0; it < TOPK_ITEMS; ++it) {
    const uint32_t c = (cls >> (2 * it)) & 3u;
    const uint64_t ms = __ballot(c == 1u), mt = __ballot(c == 2u);
    const int64_t s_before = sb + __popcll(ms & lt), t_before = tb + __popcll(mt & lt);
    if (c == 1u || (c == 2u && t_before < S.cut)) {
      const int64_t o = s_before + (t_before < S.cut ? t_before : S.cut);
      if ((uint64_t)o < (uint64_t)mout) {
        cand_out[o] = (int32_t)((uint32_t)row[it] | (c == 1u ? TOPK_SURE : 0u));
        if (c == 2u) words_out[o] = w[it];
      }
      if (c == 2u && hist) {
#pragma unroll
        for (int g = 0; g < 8; ++g) hist_add(h + 256 * g, (uint32_t)(w[it] >> (8 * g)) & 255u);
      }
    }
    sb += __popcll(ms);
    tb += __popcll(mt);
  }
  if (hist) {
    __syncthreads();
    for (int j = threadIdx.x; j < 8 * 256; j += TOPK_THREADS)
      if (h[j]) atomicAdd(&hist[j], h[j]);
  }
}

// ---- qe_take -----------------------------------------------------------------------------------
constexpr int TAKE_MAX_COLS = 8;
enum { TK_UTF8 = 0, TK_BOOL = -1 };

struct TakeCol {
  const void* in;
  const uint8_t* in_valid;
  void* out;            // TK_UTF8: int2 (source byte offset, length) per output row
  uint32_t* out_valid;  // whole 32-bit words
  int32_t width;        // 8, 4, 1, TK_UTF8 or TK_BOOL
  int32_t pad;
  const int32_t* in_offs;
};

struct TakeArgs {
  TakeCol cols[TAKE_MAX_COLS];
  int32_t ncols;
};

// A wave's 64 result bits -> the two 32-bit words of rows [64 c, 64 c + 64) (bitmaps hold nwords words).
__device__ __forceinline__ void store_bits64(uint32_t* __restrict__ bm, int64_t c, int64_t nwords, uint64_t bits, int lane) {
  if (lane == 0 && 2 * c < nwords) bm[2 * c] = (uint32_t)bits;
  if (lane == 1 && 2 * c + 1 < nwords) bm[2 * c + 1] = (uint32_t)(bits >> 32);
}

// Output row i = input row idx[i], one row per lane. An index outside [0, nin) reads nothing: the
// row gets a zero value and a null bit, and *flag is set. OR_NULL (qe_take_or_null): index -1 means
// "no row" and is written the same way without setting the flag.
template <bool OR_NULL>
__global__ void __launch_bounds__(256) k_take(const int32_t* __restrict__ idx, int64_t m, int64_t nin, TakeArgs A,
                                              unsigned* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (m + 63) >> 6, nwords = (m + 31) >> 5;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave; c < nchunks; c += nwaves) {  // the same trip count in every lane of a wave
    const int64_t i = c * 64 + lane;
    const bool live = i < m;
    const int64_t r = live ? (int64_t)idx[i] : 0;
    const bool ok = live && (uint64_t)r < (uint64_t)nin;
    if (live && !ok && !(OR_NULL && r == -1)) *flag = 1u;
    for (int k = 0; k < A.ncols; ++k) {
      const TakeCol& C = A.cols[k];
      if (C.width == 8) {
        const uint64_t v = ok ? ((const uint64_t*)C.in)[r] : 0;
        if (live) ((uint64_t*)C.out)[i] = v;
      } else if (C.width == 4) {
        const uint32_t v = ok ? ((const uint32_t*)C.in)[r] : 0;
        if (live) ((uint32_t*)C.out)[i] = v;
      } else if (C.width == 1) {
        const uint8_t v = ok ? ((const uint8_t*)C.in)[r] : 0;
        if (live) ((uint8_t*)C.out)[i] = v;
      } else if (C.width == TK_UTF8) {
        int2 e = make_int2(0, 0);
        if (ok) {
          e.x = C.in_offs[r];
          e.y = max(C.in_offs[r + 1] - e.x, 0);
        }
        if (live) ((int2*)C.out)[i] = e;
      } else {  // TK_BOOL
        const bool b = ok && ((((const uint8_t*)C.in)[r >> 3] >> (r & 7)) & 1);
        store_bits64((uint32_t*)C.out, c, nwords, __ballot(b), lane);
      }
      if (C.out_valid) {
        const bool v = ok && (!C.in_valid || ((C.in_valid[r >> 3] >> (r & 7)) & 1));
        store_bits64(C.out_valid, c, nwords, __ballot(v), lane);
      }
    }
  }
}

struct DevBlock {  // working memory of one call: freed stream-ordered when the call returns
  qe_ctx* ctx;
  void* p = nullptr;
  explicit DevBlock(qe_ctx* c) : ctx(c) {}
  ~DevBlock() { dev_free(ctx, p); }
};

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The multi-workgroup passes for other translation units (qe_join.hip orders build rows by slot):
// a stable sort of n (word, index) pairs by the low `bits` bits of the words, between the two
// buffers of each kind, starting in buffer 0. *cur = the buffer that holds the sorted indices (the
// words of the last pass are not written). `scratch`: sort_pairs_scratch_bytes(n) bytes.
size_t sort_pairs_scratch_bytes(int64_t n) {
  const int64_t ntiles = (int64_t)div_up((uint64_t)std::max<int64_t>(n, 1), SORT_TILE);
  return 2 * align256((size_t)(256 * ntiles + 1) * 8);
}

int sort_pairs(qe_ctx* ctx, uint64_t* const words[2], int32_t* const idx[2], int64_t n, int bits, void* scratch, int* cur) {
  *cur = 0;
  if (n <= 0) return QE_OK;
  const int64_t ntiles = (int64_t)div_up((uint64_t)n, SORT_TILE);
  int64_t* d_counts = (int64_t*)scratch;
  int64_t* d_offs = (int64_t*)((char*)scratch + sort_pairs_scratch_bytes(n) / 2);
  const int nd = (bits + 7) / 8;
  for (int j = 0; j < nd; ++j) {
    const int shift = 8 * j, c = *cur;
    hipLaunchKernelGGL(k_sort_count, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, words[c], n, shift, ntiles,
                       d_counts);
    QE_TRY(launch_check("k_sort_count"));
    QE_TRY(exclusive_scan_i64(ctx, d_counts, d_offs, 256 * ntiles));
    hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, words[c], idx[c],
                       j + 1 < nd ? words[c ^ 1] : (uint64_t*)nullptr, idx[c ^ 1], n, shift, ntiles, d_offs);
    QE_TRY(launch_check("k_sort_scatter"));
    *cur = c ^ 1;
  }
  return QE_OK;
}

// ---- host side of qe_sort_indices / qe_topk_indices -------------------------------------------------
// Argument rules of both calls (`who`: the one that reports) up to the output column's type; *n_out =
// the row count.
static int sort_check_args(const char* who, const qe_column* keys, const int32_t* flags, int32_t nkeys, const qe_column* out_indices,
                           int64_t* n_out) {
  QE_CHECK(nkeys >= 1 && nkeys <= QE_MAX_KEYS, QE_ERR_INVALID_ARG, "%s: 1..%d keys, got %d", who, QE_MAX_KEYS, nkeys);
  QE_CHECK(keys && flags && out_indices, QE_ERR_INVALID_ARG, "%s: null keys, flags or output", who);
  const int64_t n = keys[0].length;
  QE_CHECK(n >= 0 && n < ((int64_t)1 << 31), QE_ERR_INVALID_ARG, "%s: %lld rows (at most 2^31 - 1)", who, (long long)n);
  for (int q = 0; q < nkeys; ++q) {
    const qe_column& c = keys[q];
    QE_CHECK(c.length == n, QE_ERR_INVALID_ARG, "%s: key %d has %lld rows, key 0 %lld", who, q, (long long)c.length,
             (long long)n);
    QE_CHECK((flags[q] & ~(QE_SORT_DESC | QE_SORT_NULLS_FIRST)) == 0, QE_ERR_INVALID_ARG,
             "%s: key %d has unknown flag bits 0x%x", who, q, flags[q]);
    QE_CHECK(sort_value_bits(c.type) > 0 || c.type == QE_TYPE_UTF8, QE_ERR_UNSUPPORTED, "%s: key %d type %d", who, q, c.type);
    QE_CHECK(c.values || n == 0, QE_ERR_INVALID_ARG, "%s: key %d has no values", who, q);
    QE_CHECK(c.type != QE_TYPE_UTF8 || c.offsets || n == 0, QE_ERR_INVALID_ARG, "%s: UTF8 key %d needs offsets", who, q);
  }
  QE_CHECK(out_indices->type == QE_TYPE_INT32 && !out_indices->validity, QE_ERR_INVALID_ARG,
           "%s: the indices column must be INT32 without validity", who);
  *n_out = n;
  return QE_OK;
}

// The output column holds the m result rows; its length is set.
static int sort_check_out(const char* who, qe_column* out_indices, int64_t m) {
  QE_CHECK(out_indices->length >= m, QE_ERR_CAPACITY, "%s: the indices column holds %lld rows, need %lld", who,
           (long long)out_indices->length, (long long)m);
  QE_CHECK(out_indices->values || m == 0, QE_ERR_INVALID_ARG, "%s: the indices column has no values", who);
  out_indices->length = m;
  return QE_OK;
}

// One call's working memory, carved from one block:
// [err word + UTF8 lengths | histograms | 2 x words | 2 x indices | counts | offsets]
constexpr size_t SORT_HEAD = 256, SORT_HIST_B = 8 * 256 * 4;
struct SortMem {
  const char* who;  // the entry point, for its error messages
  char* base;  // head[0]: error word; head[4 + 4 q]: longest value of UTF8 key q
  unsigned* err;
  uint32_t* hist;
  uint64_t* words[2];
  int32_t* idx[2];
  int64_t *counts, *offs;
  void* hp;  // pinned: the head and the histograms as read back
  const unsigned* h_err;
  const uint32_t* h_hist;
  int64_t readbacks = 0;
};

// rows: entries of each pair buffer; cnt: entries of each of the two counter arrays (0: none).
static int sort_mem(qe_ctx* ctx, DevBlock& blk, int64_t rows, int64_t cnt, SortMem* M) {
  const size_t words_b = rows ? align256((size_t)rows * 8) : 0, idx_b = rows ? align256((size_t)rows * 4) : 0;
  const size_t cnt_b = cnt ? align256((size_t)cnt * 8) : 0;
  QE_TRY(dev_alloc(ctx, SORT_HEAD + SORT_HIST_B + 2 * words_b + 2 * idx_b + 2 * cnt_b, &blk.p));
  char* base = (char*)blk.p;
  M->base = base;
  M->err = (unsigned*)base;
  M->hist = (uint32_t*)(base + SORT_HEAD);
  char* p = base + SORT_HEAD + SORT_HIST_B;
  M->words[0] = (uint64_t*)p;
  M->words[1] = (uint64_t*)(p + words_b);
  M->idx[0] = (int32_t*)(p + 2 * words_b);
  M->idx[1] = (int32_t*)(p + 2 * words_b + idx_b);
  M->counts = (int64_t*)(p + 2 * words_b + 2 * idx_b);
  M->offs = (int64_t*)((char*)M->counts + cnt_b);
  QE_HIP(hipMemsetAsync(base, 0, SORT_HEAD, ctx->stream));
  QE_TRY(ctx_pinned(ctx, SORT_HEAD + SORT_HIST_B, &M->hp));
  M->h_err = (const unsigned*)M->hp;
  M->h_hist = (const uint32_t*)((char*)M->hp + SORT_HEAD);
  return QE_OK;
}

// The head and the histograms come back; a broken short-UTF8 promise fails the call here.
static int sort_read_back(qe_ctx* ctx, SortMem& M, size_t bytes) {
  QE_HIP(hipMemcpyAsync(M.hp, M.base, bytes, hipMemcpyDeviceToHost, ctx->stream));
  QE_TRY(ctx_sync(ctx));
  ++M.readbacks;
  QE_CHECK(M.h_err[0] == 0, QE_ERR_INVALID_ARG, "%s: a UTF8 key value is longer than the column's max_len", M.who);
  return QE_OK;
}

// The key layout of a call. *promised: a UTF8 key relies on max_len (the device checks the bound).
static int sort_build_desc(qe_ctx* ctx, const qe_column* keys, const int32_t* flags, int32_t nkeys, int64_t n, SortMem& M,
                           SortDesc* D_out, bool* promised_out) {
  // UTF8 keys without a bound of at most 7 bytes: the longest value, one reduction each, one read-back
  int64_t longest[QE_MAX_KEYS] = {};
  bool promised = false, reduced = false;
  for (int q = 0; q < nkeys; ++q) {
    if (keys[q].type != QE_TYPE_UTF8) continue;
    if (keys[q].max_len >= 1 && keys[q].max_len <= 7) {
      longest[q] = keys[q].max_len;
      promised = true;
      continue;
    }
    const int grid = (int)std::min<int64_t>((int64_t)div_up((uint64_t)n, 256), (int64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(k_utf8_max_len, dim3(grid), dim3(256), 0, ctx->stream, keys[q].offsets, n,
                       (int32_t*)M.base + 4 + 4 * q);
    QE_TRY(launch_check("k_utf8_max_len"));
    reduced = true;
  }
  if (reduced) {
    QE_HIP(hipMemcpyAsync(M.hp, M.base, SORT_HEAD, hipMemcpyDeviceToHost, ctx->stream));
    QE_TRY(ctx_sync(ctx));
    ++M.readbacks;
    for (int q = 0; q < nkeys; ++q)
      if (keys[q].type == QE_TYPE_UTF8 && !(keys[q].max_len >= 1 && keys[q].max_len <= 7))
        longest[q] = ((const int32_t*)M.hp)[4 + 4 * q];
  }

  // key layout, from the least significant bit: the last key first
  SortDesc D{};
  D.nkeys = nkeys;
  int64_t lo = 0;
  for (int q = nkeys - 1; q >= 0; --q) {
    const qe_column& c = keys[q];
    SortKey& K = D.key[q];
    K.values = c.values;
    K.validity = c.validity;
    K.offsets = c.offsets;
    K.type = c.type;
    K.flags = flags[q];
    K.lo_v = lo;
    if (c.type != QE_TYPE_UTF8) {
      K.mode = SK_FIXED;
      K.vbits = sort_value_bits(c.type);
      lo += K.vbits;
    } else if (longest[q] <= 7) {
      K.mode = SK_UTF8_SHORT;
      K.vbits = 64;
      lo += 64;
    } else {
      K.mode = SK_UTF8;
      K.vbits = 32;  // the byte length, below the chunks: the last tiebreak
      lo = (lo + 32 + 63) & ~(int64_t)63;
      K.cw0 = lo / 64;
      K.nchunks = (longest[q] + 7) / 8;
      lo += 64 * K.nchunks;
    }
    K.lo_n = -1;
    if (c.validity) K.lo_n = lo++;
  }
  const int64_t nwords = (lo + 63) / 64;
  QE_CHECK(nwords <= SORT_MAX_WORDS, QE_ERR_UNSUPPORTED, "%s: the keys take %lld bytes per row (at most %lld)", M.who,
           (long long)nwords * 8, (long long)SORT_MAX_WORDS * 8);
  D.nwords = (int32_t)nwords;
  *D_out = D;
  *promised_out = promised;
  return QE_OK;
}

// The multi-workgroup sort of m rows of a column of nrows: per word, the encode through the current
// permutation and the passes of its varying digits. list: the rows are the m entries of M.idx[cur]
// (a top-k candidate list, flag bits included); otherwise rows 0 .. m - 1 (m == nrows). *cur_out =
// the index buffer that holds the order.
static int sort_multi(qe_ctx* ctx, const SortDesc& D, int64_t nrows, int64_t m, bool list, SortMem& M, int cur,
                      int* cur_out) {
  const int64_t ntiles = (int64_t)div_up((uint64_t)m, SORT_TILE);
  const int egrid = (int)std::min<int64_t>((int64_t)div_up((uint64_t)m, ENC_THREADS), (int64_t)ctx->num_cus * 8);
  for (int64_t k = 0; k < D.nwords; ++k) {
    QE_HIP(hipMemsetAsync(M.hist, 0, SORT_HIST_B, ctx->stream));
    if (list) {
      hipLaunchKernelGGL(k_topk_words<TW_SORT>, dim3(egrid), dim3(ENC_THREADS), 0, ctx->stream, D, k, nrows, m, M.idx[cur],
                         M.words[cur], k == 0 ? 1 : 0, M.hist, M.err);
      QE_TRY(launch_check("k_topk_words"));
    } else {
      hipLaunchKernelGGL(k_sort_encode, dim3(egrid), dim3(ENC_THREADS), 0, ctx->stream, D, k, m,
                         k == 0 ? (const int32_t*)nullptr : (const int32_t*)M.idx[cur], M.words[cur],
                         k == 0 ? M.idx[cur] : (int32_t*)nullptr, M.hist, M.err);
      QE_TRY(launch_check("k_sort_encode"));
    }
    QE_TRY(sort_read_back(ctx, M, SORT_HEAD + SORT_HIST_B));
    int digits[8], nd = 0;
    for (int g = 0; g < 8; ++g) {
      bool constant = false;
      for (int v = 0; v < 256; ++v) constant |= M.h_hist[256 * g + v] == (uint32_t)m;
      if (!constant) digits[nd++] = g;
    }
    for (int j = 0; j < nd; ++j) {
      const int shift = 8 * digits[j];
      hipLaunchKernelGGL(k_sort_count, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, M.words[cur], m, shift,
                         ntiles, M.counts);
      QE_TRY(launch_check("k_sort_count"));
      QE_TRY(exclusive_scan_i64(ctx, M.counts, M.offs, 256 * ntiles));
      hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, M.words[cur],
                         M.idx[cur], j + 1 < nd ? M.words[cur ^ 1] : (uint64_t*)nullptr, M.idx[cur ^ 1], m, shift, ntiles,
                         M.offs);
      QE_TRY(launch_check("k_sort_scatter"));
      cur ^= 1;
    }
  }
  *cur_out = cur;
  return QE_OK;
}

// qe_sort_indices (and qe_topk_indices' QE_TOPK_SORT, which reports as `who`); *readbacks (may be
// NULL) = the host read-backs of the call.
static int sort_impl(qe_ctx* ctx, const char* who, const qe_column* keys, const int32_t* flags, int32_t nkeys,
                     int64_t limit, qe_column* out_indices, int64_t* readbacks) {
  int64_t n;
  QE_TRY(sort_check_args(who, keys, flags, nkeys, out_indices, &n));
  const int64_t m = limit < 0 ? n : std::min(limit, n);
  QE_TRY(sort_check_out(who, out_indices, m));
  if (m == 0) return QE_OK;

  const bool small = n <= SORT_SMALL_MAX;
  const int64_t ntiles = (int64_t)div_up((uint64_t)n, SORT_TILE);
  DevBlock blk(ctx);
  SortMem M;
  M.who = who;
  QE_TRY(sort_mem(ctx, blk, small ? 0 : n, small ? 0 : 256 * ntiles + 1, &M));
  SortDesc D;
  bool promised;
  int st = sort_build_desc(ctx, keys, flags, nkeys, n, M, &D, &promised);
  if (st == QE_OK && small) {
    hipLaunchKernelGGL(k_sort_small, dim3(1), dim3(SORT_SMALL_THREADS), 0, ctx->stream, D, (int32_t)n, (int32_t)m,
                       (int32_t*)out_indices->values, M.err);
    st = launch_check("k_sort_small");
    if (st == QE_OK && promised) st = sort_read_back(ctx, M, 4);  // (nothing else of this path needs the host)
  } else if (st == QE_OK) {
    int cur = 0;
    st = sort_multi(ctx, D, n, n, false, M, 0, &cur);
    if (st == QE_OK && hipMemcpyAsync(out_indices->values, M.idx[cur], (size_t)m * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
      st = fail(QE_ERR_DEVICE, "%s: copying the indices failed", who);
  }
  if (readbacks) *readbacks = M.readbacks;
  return st;
}

// The top-k's two (word, index) candidate buffers of `rows` entries each, in a block of their own:
// they are sized once the first pick has bounded the candidates, after the block of sort_mem.
static int topk_mem_pairs(qe_ctx* ctx, DevBlock& blk, int64_t rows, SortMem* M) {
  const size_t words_b = align256((size_t)rows * 8), idx_b = align256((size_t)rows * 4);
  QE_TRY(dev_alloc(ctx, 2 * words_b + 2 * idx_b, &blk.p));
  char* p = (char*)blk.p;
  M->words[0] = (uint64_t*)p;
  M->words[1] = (uint64_t*)(p + words_b);
  M->idx[0] = (int32_t*)(p + 2 * words_b);
  M->idx[1] = (int32_t*)(p + 2 * words_b + idx_b);
  return QE_OK;
}

// The 8 digit histograms of word kw over the tied rows of the `cand` candidates in M.idx[cur] /
// M.words[cur] (implicit: over all n rows, and nothing else is written), read back.
static int topk_histogram(qe_ctx* ctx, const SortDesc& D, int64_t kw, int64_t n, bool implicit, int64_t cand, SortMem& M,
                          int cur) {
  const int egrid = (int)std::min<int64_t>((int64_t)div_up((uint64_t)cand, ENC_THREADS), (int64_t)ctx->num_cus * 8);
  QE_HIP(hipMemsetAsync(M.hist, 0, SORT_HIST_B, ctx->stream));
  if (implicit)
    hipLaunchKernelGGL(k_topk_words<TW_ALL>, dim3(egrid), dim3(ENC_THREADS), 0, ctx->stream, D, kw, n, n, (int32_t*)nullptr,
                       (uint64_t*)nullptr, 0, M.hist, M.err);
  else
    hipLaunchKernelGGL(k_topk_words<TW_TIED>, dim3(egrid), dim3(ENC_THREADS), 0, ctx->stream, D, kw, n, cand, M.idx[cur],
                       M.words[cur], 0, M.hist, M.err);
  QE_TRY(launch_check("k_topk_words"));
  return sort_read_back(ctx, M, SORT_HEAD + SORT_HIST_B);
}

// One digit step (or the final cut) of the selection: the m candidates of M.idx[cur] / M.words[cur]
// (implicit: rows 0 .. m - 1) that stay under S go to the other buffers (implicit: buffers 0), mout
// of them. want_hist: M.hist receives the histograms of the rows that stay tied.
static int topk_compact(qe_ctx* ctx, const SortDesc& D, const TopkStep& S, bool implicit, int64_t m, int64_t mout,
                        SortMem& M, int cur, bool want_hist) {
  const int64_t ntiles = (int64_t)div_up((uint64_t)m, TOPK_TILE);
  const int out = implicit ? 0 : cur ^ 1;
  uint32_t* hist = want_hist ? M.hist : nullptr;
  if (want_hist) QE_HIP(hipMemsetAsync(M.hist, 0, SORT_HIST_B, ctx->stream));
  if (implicit)
    hipLaunchKernelGGL(k_topk_count<true>, dim3((unsigned)ntiles), dim3(TOPK_THREADS), 0, ctx->stream, D, S, m,
                       (const int32_t*)nullptr, (const uint64_t*)nullptr, ntiles, M.counts, M.err);
  else
    hipLaunchKernelGGL(k_topk_count<false>, dim3((unsigned)ntiles), dim3(TOPK_THREADS), 0, ctx->stream, D, S, m,
                       (const int32_t*)M.idx[cur], (const uint64_t*)M.words[cur], ntiles, M.counts, M.err);
  QE_TRY(launch_check("k_topk_count"));
  QE_TRY(exclusive_scan_i64(ctx, M.counts, M.offs, 2 * ntiles));
  if (implicit)
    hipLaunchKernelGGL(k_topk_compact<true>, dim3((unsigned)ntiles), dim3(TOPK_THREADS), 0, ctx->stream, D, S, m,
                       (const int32_t*)nullptr, (const uint64_t*)nullptr, ntiles, (const int64_t*)M.offs, mout, M.idx[out],
                       M.words[out], hist, M.err);
  else
    hipLaunchKernelGGL(k_topk_compact<false>, dim3((unsigned)ntiles), dim3(TOPK_THREADS), 0, ctx->stream, D, S, m,
                       (const int32_t*)M.idx[cur], (const uint64_t*)M.words[cur], ntiles, (const int64_t*)M.offs, mout,
                       M.idx[out], M.words[out], hist, M.err);
  return launch_check("k_topk_compact");
}

// qe_topk_indices in selection mode: n > 0 rows, the first m = min(k, n) > 0 of the order. Everything
// here is a function of m, never of the caller's k (which may be INT64_MAX). stats[1], stats[2] =
// the digit steps and the candidates handed to the final sort; M.readbacks counts the read-backs.
static int topk_select(qe_ctx* ctx, const qe_column* keys, const int32_t* flags, int32_t nkeys, int64_t n, int64_t m,
                       int32_t* out, SortMem& M, int64_t* stats) {
  // working memory: a block of [head | histograms | tile counters] now; the candidate buffers in a
  // second block once the first pick says how many rows survive (both released stream-ordered)
  const int64_t fmax = std::min(n, std::max<int64_t>(SORT_SMALL_MAX, (int64_t)QE_TOPK_STOP_FACTOR * m));
  const int64_t cnt = n <= SORT_SMALL_MAX ? 0
                                          : std::max<int64_t>(2 * (int64_t)div_up((uint64_t)n, TOPK_TILE) + 1,
                                                              256 * (int64_t)div_up((uint64_t)fmax, SORT_TILE) + 1);
  DevBlock blk(ctx), pairs(ctx);
  QE_TRY(sort_mem(ctx, blk, 0, cnt, &M));
  SortDesc D;
  bool promised;
  QE_TRY(sort_build_desc(ctx, keys, flags, nkeys, n, M, &D, &promised));

  TopkNeed C{m, 0, n};
  bool implicit = true, have_hist = false;
  int cur = 0;
  int64_t kw = D.nwords - 1;
  while (!topk_stop(C.candidates(), m, SORT_SMALL_MAX)) {
    const int64_t before = C.candidates();
    // the highest digit, of this word or of a lower one, on which the tied rows differ
    int32_t g = -1;
    for (; kw >= 0; --kw, have_hist = false) {
      if (!have_hist) QE_TRY(topk_histogram(ctx, D, kw, n, implicit, before, M, cur));
      have_hist = true;
      g = topk_top_digit(M.h_hist, C.tied);
      if (g >= 0) break;
    }
    TopkStep S{};
    S.cut = INT64_MAX;
    if (g >= 0) {
      const TopkPick P = topk_pick_bin(M.h_hist + 256 * g, C.need());
      QE_CHECK(P.bin >= 0, QE_ERR_DEVICE, "topk: the digit histogram holds fewer rows than the selection needs");
      S.k = kw;
      S.shift = 8 * g;
      S.bin = (uint32_t)P.bin;
      C.take(P);
      ++stats[1];
    } else {  // every digit of every word is spent: the tied rows are equal, the first need() of them stay
      S.cut_only = 1;
      S.cut = C.need();
      C.cut();
    }
    have_hist = g >= 0 && !topk_stop(C.candidates(), m, SORT_SMALL_MAX);  // another step follows: it needs histograms
    if (implicit) QE_TRY(topk_mem_pairs(ctx, pairs, C.candidates(), &M));
    QE_TRY(topk_compact(ctx, D, S, implicit, before, C.candidates(), M, cur, have_hist));
    if (!implicit) cur ^= 1;
    implicit = false;
    if (have_hist) QE_TRY(sort_read_back(ctx, M, SORT_HEAD + SORT_HIST_B));
  }

  const int64_t cand = stats[2] = C.candidates();
  if (cand <= SORT_SMALL_MAX) {
    if (implicit)
      hipLaunchKernelGGL(k_sort_small, dim3(1), dim3(SORT_SMALL_THREADS), 0, ctx->stream, D, (int32_t)n, (int32_t)m, out,
                         M.err);
    else
      hipLaunchKernelGGL(k_sort_small_rows, dim3(1), dim3(SORT_SMALL_THREADS), 0, ctx->stream, D, (int32_t)cand, (int32_t)n,
                         (const int32_t*)M.idx[cur], (int32_t)m, out, M.err);
    QE_TRY(launch_check("k_sort_small"));
    if (promised) QE_TRY(sort_read_back(ctx, M, 4));
    return QE_OK;
  }
  if (implicit) QE_TRY(topk_mem_pairs(ctx, pairs, n, &M));  // no step ran: the candidates are all n rows
  QE_TRY(sort_multi(ctx, D, n, cand, !implicit, M, cur, &cur));
  QE_HIP(hipMemcpyAsync(out, M.idx[cur], (size_t)m * 4, hipMemcpyDeviceToDevice, ctx->stream));
  return QE_OK;
}

}  // namespace qe

using namespace qe;

extern "C" {

int qe_sort_layout(int32_t* tile_rows, int32_t* small_max) {
  if (tile_rows) *tile_rows = SORT_TILE;
  if (small_max) *small_max = SORT_SMALL_MAX;
  return QE_OK;
}

int qe_sort_indices(qe_ctx* ctx, const qe_column* keys, const int32_t* flags, int32_t nkeys, int64_t limit,
                    qe_column* out_indices) {
  QE_TRY(ctx_enter(ctx));
  return sort_impl(ctx, "sort", keys, flags, nkeys, limit, out_indices, nullptr);
}

int qe_topk_indices(qe_ctx* ctx, const qe_column* keys, const int32_t* flags, int32_t nkeys, int64_t k, int32_t mode,
                    qe_column* out_indices) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(k >= 0, QE_ERR_INVALID_ARG, "topk: k = %lld is negative", (long long)k);
  QE_CHECK(mode == QE_TOPK_AUTO || mode == QE_TOPK_SELECT || mode == QE_TOPK_SORT, QE_ERR_INVALID_ARG,
           "topk: unknown mode %d", mode);
  int64_t n;
  QE_TRY(sort_check_args("topk", keys, flags, nkeys, out_indices, &n));
  const int64_t m = std::min(k, n);  // from here on only m is used: k may be INT64_MAX
  const bool select = mode == QE_TOPK_SELECT ? n > 0 : mode == QE_TOPK_AUTO && topk_use_select(n, m, SORT_SMALL_MAX);
  int64_t* stats = ctx->topk_stats;
  stats[0] = select ? 1 : 0;
  stats[1] = stats[3] = 0;
  stats[2] = select ? 0 : n;
  if (!select) return sort_impl(ctx, "topk", keys, flags, nkeys, m, out_indices, &stats[3]);
  QE_TRY(sort_check_out("topk", out_indices, m));
  if (m == 0) return QE_OK;
  SortMem M;
  M.who = "topk";
  const int st = topk_select(ctx, keys, flags, nkeys, n, m, (int32_t*)out_indices->values, M, stats);
  stats[3] = M.readbacks;
  return st;
}

int qe_topk_last_stats(qe_ctx* ctx, int64_t stats[4]) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(stats != nullptr, QE_ERR_INVALID_ARG, "topk: null stats");
  for (int i = 0; i < 4; ++i) stats[i] = ctx->topk_stats[i];
  return QE_OK;
}

}  // extern "C"

// qe_take, and qe_take_or_null (or_null: index -1 is "no row", and every output needs a validity buffer).
static int take_impl(qe_ctx* ctx, const qe_column* indices, const qe_column* inputs, int32_t ncols, qe_column* outs,
                     const int64_t* utf8_capacity, bool or_null) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(indices != nullptr, QE_ERR_INVALID_ARG, "take: null indices");
  QE_CHECK(indices->type == QE_TYPE_INT32 && !indices->validity, QE_ERR_INVALID_ARG,
           "take: the indices column must be INT32 without validity");
  QE_CHECK(ncols >= 0 && ncols <= TAKE_MAX_COLS, QE_ERR_UNSUPPORTED, "take: at most %d columns per call", TAKE_MAX_COLS);
  QE_CHECK(ncols == 0 || (inputs && outs), QE_ERR_INVALID_ARG, "take: null column arrays");
  const int64_t m = indices->length;
  QE_CHECK(m >= 0 && (indices->values || m == 0), QE_ERR_INVALID_ARG, "take: the indices column has no values");
  const int64_t nin = ncols ? inputs[0].length : 0;
  TakeArgs args{};
  args.ncols = ncols;
  int nutf8 = 0;
  for (int i = 0; i < ncols; ++i) {
    const qe_column& in = inputs[i];
    const qe_column& out = outs[i];
    const bool utf8 = in.type == QE_TYPE_UTF8, boolean = in.type == QE_TYPE_BOOL;
    QE_CHECK(is_fixed(in.type) || utf8 || boolean, QE_ERR_UNSUPPORTED, "take: column %d type %d not supported", i, in.type);
    QE_CHECK(in.length == nin && nin >= 0, QE_ERR_INVALID_ARG, "take: column %d has %lld rows, column 0 %lld", i,
             (long long)in.length, (long long)nin);
    QE_CHECK(in.values || nin == 0, QE_ERR_INVALID_ARG, "take: column %d has no values", i);
    QE_CHECK(out.type == in.type && (out.values || m == 0), QE_ERR_INVALID_ARG, "take: output %d must have the input's type", i);
    QE_CHECK(out.length >= m, QE_ERR_CAPACITY, "take: output %d holds %lld rows, need %lld", i, (long long)out.length,
             (long long)m);
    QE_CHECK((!in.validity || out.validity) && ((uintptr_t)out.validity & 3) == 0, QE_ERR_INVALID_ARG,
             "take: output %d needs a 4-byte aligned validity buffer", i);
    QE_CHECK(!or_null || out.validity, QE_ERR_INVALID_ARG, "take: output %d needs a validity buffer (index -1 gives a null row)", i);
    QE_CHECK(!boolean || ((uintptr_t)out.values & 3) == 0, QE_ERR_INVALID_ARG, "take: BOOL output %d must be 4-byte aligned", i);
    QE_CHECK(!utf8 || ((in.offsets || nin == 0) && out.offsets), QE_ERR_INVALID_ARG, "take: UTF8 column %d needs offsets", i);
    QE_CHECK(!utf8 || (utf8_capacity && utf8_capacity[i] >= 0), QE_ERR_INVALID_ARG,
             "take: UTF8 output %d needs its values capacity (utf8_capacity)", i);
    args.cols[i] = TakeCol{in.values, in.validity, out.values, out.validity ? (uint32_t*)out.validity : nullptr,
                           utf8 ? TK_UTF8 : boolean ? TK_BOOL : type_width(in.type), 0, utf8 ? in.offsets : nullptr};
    // an output validity buffer without an input one is filled too: all valid, nulls for bad indices
    nutf8 += utf8;
  }
  if (m == 0) {
    for (int i = 0; i < ncols; ++i) {
      if (inputs[i].type == QE_TYPE_UTF8) QE_HIP(hipMemsetAsync(outs[i].offsets, 0, 4, ctx->stream));
      outs[i].length = 0;
    }
    return QE_OK;
  }
  // working memory: [flag | per UTF8 column: (start, length) pairs, tile sums and offsets]
  const int64_t stiles = utf8_gather_tiles(m);
  const size_t pairs_b = align256((size_t)m * sizeof(int2)), tsum_b = align256((size_t)(2 * stiles + 1) * 8);
  DevBlock blk(ctx);
  QE_TRY(dev_alloc(ctx, 256 + (size_t)nutf8 * (pairs_b + tsum_b), &blk.p));
  char* base = (char*)blk.p;
  unsigned* d_flag = (unsigned*)base;
  QE_HIP(hipMemsetAsync(d_flag, 0, 4, ctx->stream));
  const int2* pairs[TAKE_MAX_COLS] = {};
  int64_t* tsum[TAKE_MAX_COLS] = {};
  for (int i = 0, u = 0; i < ncols; ++i) {
    if (args.cols[i].width != TK_UTF8) continue;
    char* p = base + 256 + (size_t)u++ * (pairs_b + tsum_b);
    pairs[i] = (const int2*)p;
    tsum[i] = (int64_t*)(p + pairs_b);
    args.cols[i].out = p;
  }
  if (ncols > 0) {
    const int grid = (int)std::min<int64_t>((int64_t)div_up((uint64_t)m, 256), (int64_t)ctx->num_cus * 8);
    if (or_null)
      hipLaunchKernelGGL(k_take<true>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t*)indices->values, m, nin, args,
                         d_flag);
    else
      hipLaunchKernelGGL(k_take<false>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t*)indices->values, m, nin, args,
                         d_flag);
    QE_TRY(launch_check("k_take"));
  }
  // the flag and the UTF8 byte totals come back together, before any byte is copied
  void* hp;
  QE_TRY(ctx_pinned(ctx, 8 * (1 + TAKE_MAX_COLS), &hp));
  int64_t* h = (int64_t*)hp;
  QE_HIP(hipMemcpyAsync(h, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  for (int i = 0; i < ncols; ++i) {
    if (!pairs[i]) continue;
    QE_TRY(utf8_gather_lengths(ctx, pairs[i], m, tsum[i]));
    QE_HIP(hipMemcpyAsync(h + 1 + i, tsum[i] + 2 * stiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  QE_TRY(ctx_sync(ctx));
  QE_CHECK(*(const unsigned*)h == 0, QE_ERR_INVALID_ARG,
           "take: an index is outside [0, %lld) (its row was written as null / zero)", (long long)nin);
  for (int i = 0; i < ncols; ++i) {
    if (!pairs[i]) continue;
    QE_CHECK(h[1 + i] < ((int64_t)1 << 31), QE_ERR_UNSUPPORTED, "take: UTF8 output %d needs %lld bytes (int32 offsets)", i,
             (long long)h[1 + i]);
    QE_CHECK(h[1 + i] <= utf8_capacity[i], QE_ERR_CAPACITY, "take: UTF8 output %d holds %lld bytes, need %lld", i,
             (long long)utf8_capacity[i], (long long)h[1 + i]);
  }
  for (int i = 0; i < ncols; ++i)
    if (pairs[i])
      QE_TRY(utf8_gather_copy(ctx, pairs[i], m, tsum[i], (const uint8_t*)inputs[i].values, outs[i].offsets,
                              (uint8_t*)outs[i].values));
  for (int i = 0; i < ncols; ++i) outs[i].length = m;
  return QE_OK;
}

extern "C" {

int qe_take(qe_ctx* ctx, const qe_column* indices, const qe_column* inputs, int32_t ncols, qe_column* outs,
            const int64_t* utf8_capacity) {
  return take_impl(ctx, indices, inputs, ncols, outs, utf8_capacity, false);
}

int qe_take_or_null(qe_ctx* ctx, const qe_column* indices, const qe_column* inputs, int32_t ncols, qe_column* outs,
                    const int64_t* utf8_capacity) {
  return take_impl(ctx, indices, inputs, ncols, outs, utf8_capacity, true);
}

}  // extern "C"
