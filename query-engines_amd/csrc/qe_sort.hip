// ORDER BY (build-defined operator): stable multi-key sort to row indices, and
// the first k rows of that order (qe_take.hip gathers by the indices).
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
// sort_pairs
//   the count / scan / scatter passes over a caller's (word, index) buffers (qe_join.hip).
// One body each serves the two encoders (encode_words), the two small sorts (sort_small) and every
// digit pass (sort_digit_pass).
#include "qe_rows.hpp"
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
    const bool valid = row_valid(K.validity, r);
    if (in_n) w |= sort_null_bit(valid, K.flags) << (K.lo_n - b0);
    if (!valid) continue;
    if (K.mode == SK_FIXED) {
      const uint64_t raw = load_fixed_raw(K.type, K.values, r);
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

// A workgroup's 8 digit histograms of a word in LDS: cleared, filled by hist_add, then added to the
// global ones (the caller puts a barrier between the steps).
template <int THREADS>
__device__ __forceinline__ void hist_clear(uint32_t* h) {
  for (int j = threadIdx.x; j < 8 * 256; j += THREADS) h[j] = 0;
}
template <int THREADS>
__device__ __forceinline__ void hist_flush(const uint32_t* h, uint32_t* __restrict__ hist) {
  for (int j = threadIdx.x; j < 8 * 256; j += THREADS)
    if (h[j]) atomicAdd(&hist[j], h[j]);
}

// Word k of the rows that m list entries name, and hist[256 g + v] += encoded rows whose digit g of
// that word is v. The list:
//   TW_PERM : the sort's permutation `list` of rows 0 .. m - 1 -> words[i]; list NULL: row i, and
//             iota[i] = i
//   TW_ALL  : the top-k's implicit list, rows 0 .. m - 1; nothing but the histograms is written
//   TW_TIED : the tied entries of the candidate list (top-k section below) -> words[i]
//   TW_SORT : every entry of the candidate list -> words[i]; `strip`: the flag bits leave `list` (the
//             final sort's first word: from here on the list is the sort's permutation)
constexpr uint32_t TOPK_SURE = 0x80000000u;
constexpr int ENC_THREADS = 256;
enum { TW_ALL = 0, TW_TIED = 1, TW_SORT = 2, TW_PERM = 3 };
template <int MODE>
__device__ __forceinline__ void encode_words(const SortDesc& D, int64_t k, int64_t nrows, int64_t m,
                                             int32_t* __restrict__ list, uint64_t* __restrict__ words,
                                             int32_t* __restrict__ iota, int strip, uint32_t* __restrict__ hist,
                                             unsigned* __restrict__ err) {
  __shared__ uint32_t h[8 * 256];
  hist_clear<ENC_THREADS>(h);
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)ENC_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * ENC_THREADS) {
    int64_t r = i;
    if (MODE == TW_PERM) {
      if (list) r = (int64_t)list[i];
    } else if (MODE != TW_ALL) {
      const uint32_t c = (uint32_t)list[i];
      if (MODE == TW_TIED && (c & TOPK_SURE)) continue;
      r = (int64_t)(c & ~TOPK_SURE);
      if (MODE == TW_SORT && strip) list[i] = (int32_t)r;
    }
    if ((uint64_t)r >= (uint64_t)nrows) r = 0;  // (a permutation or a candidate never is)
    const uint64_t w = sort_word(D, r, k, err);
    if (MODE != TW_ALL) words[i] = w;
    if (MODE == TW_PERM && iota) iota[i] = (int32_t)i;
#pragma unroll
    for (int g = 0; g < 8; ++g) hist_add(h + 256 * g, (uint32_t)(w >> (8 * g)) & 255u);
  }
  __syncthreads();
  hist_flush<ENC_THREADS>(h, hist);
}

__global__ void __launch_bounds__(ENC_THREADS) k_sort_encode(SortDesc D, int64_t k, int64_t n,
                                                              const int32_t* __restrict__ perm,
                                                              uint64_t* __restrict__ words, int32_t* __restrict__ idx_out,
                                                              uint32_t* __restrict__ hist, unsigned* __restrict__ err) {
  encode_words<TW_PERM>(D, k, n, n, const_cast<int32_t*>(perm), words, idx_out, 0, hist, err);  // (TW_PERM only reads it)
}

template <int MODE>
__global__ void __launch_bounds__(ENC_THREADS) k_topk_words(SortDesc D, int64_t k, int64_t nrows, int64_t m,
                                                             int32_t* __restrict__ cand, uint64_t* __restrict__ words,
                                                             int strip, uint32_t* __restrict__ hist,
                                                             unsigned* __restrict__ err) {
  encode_words<MODE>(D, k, nrows, m, cand, words, nullptr, strip, hist, err);
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
// passes between two LDS pair buffers. out[0 .. m_out) = the first rows of the order. LIST (the
// top-k's final sort): the rows are the n entries of `rows` (row indices below nrows, flag bit 31
// ignored), not 0 .. n - 1 (nrows == n), and rows that compare equal keep the list's order.
template <bool LIST>
__device__ __forceinline__ void sort_small(const SortDesc& D, int32_t n, int32_t nrows, const int32_t* __restrict__ rows,
                                           int32_t m_out, int32_t* __restrict__ out, unsigned* __restrict__ err) {
  __shared__ uint64_t s_word[2][SORT_SMALL_MAX];
  __shared__ int32_t s_idx[2][SORT_SMALL_MAX];
  constexpr int WAVES = SORT_SMALL_THREADS / 64;
  __shared__ uint16_t s_wcnt[WAVES][256];
  __shared__ uint32_t s_dstart[256];
  __shared__ uint32_t s_wsum[4];
  __shared__ uint64_t s_or[WAVES], s_and[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int cur = 0;
  for (int p = threadIdx.x; p < n; p += SORT_SMALL_THREADS) s_idx[0][p] = LIST ? rows[p] & 0x7FFFFFFF : p;
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

__global__ void __launch_bounds__(SORT_SMALL_THREADS) k_sort_small(SortDesc D, int32_t n, int32_t m_out,
                                                             int32_t* __restrict__ out, unsigned* __restrict__ err) {
  sort_small<false>(D, n, n, nullptr, m_out, out, err);
}

__global__ void __launch_bounds__(SORT_SMALL_THREADS) k_sort_small_rows(SortDesc D, int32_t n, int32_t nrows,
                                                                  const int32_t* __restrict__ rows, int32_t m_out,
                                                                  int32_t* __restrict__ out, unsigned* __restrict__ err) {
  sort_small<true>(D, n, nrows, rows, m_out, out, err);
}

// ---- top-k: radix selection (qe_topk_plan.hpp holds the host's rules) ------------------------------
// The candidate list: row indices in ascending row order, bit 31 set on a sure row. A tied row's
// current key word lies beside it; a sure row's word is never read again. Before the first
// compaction the list is implicit: every row, all tied.
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_ITEMS = 16;
constexpr int TOPK_TILE = TOPK_THREADS * TOPK_ITEMS;  // candidates per workgroup of a compaction
static_assert(TOPK_TILE == SORT_TILE, "qe_sort_layout reports one tile size");

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
  if (hist) hist_clear<TOPK_THREADS>(h);
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
    hist_flush<TOPK_THREADS>(h, hist);
  }
}

// ---- the multi-workgroup digit pass -----------------------------------------------------------------
// One stable pass over n (word, index) pairs by the digit at `shift`: tile counts, their scan, the
// scatter from (win, iin) to (wout, iout). wout NULL: the last pass, whose words nobody reads.
// counts, offs: 256 tiles + 1 entries each.
static int sort_digit_pass(qe_ctx* ctx, const uint64_t* win, const int32_t* iin, uint64_t* wout, int32_t* iout, int64_t n,
                           int shift, int64_t* counts, int64_t* offs) {
  const int64_t ntiles = (int64_t)div_up((uint64_t)n, SORT_TILE);
  hipLaunchKernelGGL(k_sort_count, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, win, n, shift, ntiles, counts);
  QE_TRY(launch_check("k_sort_count"));
  QE_TRY(exclusive_scan_i64(ctx, counts, offs, 256 * ntiles));
  hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)ntiles), dim3(SORT_THREADS), 0, ctx->stream, win, iin, wout, iout, n, shift,
                     ntiles, (const int64_t*)offs);
  return launch_check("k_sort_scatter");
}

// The passes for other translation units (qe_join.hip orders build rows by slot): a stable sort of
// n (word, index) pairs by the low `bits` bits of the words, between the two buffers of each kind,
// starting in buffer 0. *cur = the buffer that holds the sorted indices (the words of the last pass
// are not written). `scratch`: sort_pairs_scratch_bytes(n) bytes.
size_t sort_pairs_scratch_bytes(int64_t n) {
  const int64_t ntiles = (int64_t)div_up((uint64_t)std::max<int64_t>(n, 1), SORT_TILE);
  return 2 * align256((size_t)(256 * ntiles + 1) * 8);
}

int sort_pairs(qe_ctx* ctx, uint64_t* const words[2], int32_t* const idx[2], int64_t n, int bits, void* scratch, int* cur) {
  *cur = 0;
  if (n <= 0) return QE_OK;
  int64_t* d_counts = (int64_t*)scratch;
  int64_t* d_offs = (int64_t*)((char*)scratch + sort_pairs_scratch_bytes(n) / 2);
  const int nd = (bits + 7) / 8;
  for (int j = 0; j < nd; ++j) {
    const int c = *cur;
    QE_TRY(sort_digit_pass(ctx, words[c], idx[c], j + 1 < nd ? words[c ^ 1] : nullptr, idx[c ^ 1], n, 8 * j, d_counts, d_offs));
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

// The two word and two index buffers of `rows` entries each (0: none): their bytes, and their places
// from p on; returns the first byte behind them.
static size_t pairs_bytes(int64_t rows) { return 2 * align256((size_t)rows * 8) + 2 * align256((size_t)rows * 4); }
static char* carve_pairs(char* p, int64_t rows, SortMem* M) {
  const size_t words_b = align256((size_t)rows * 8), idx_b = align256((size_t)rows * 4);
  M->words[0] = (uint64_t*)p;
  M->words[1] = (uint64_t*)(p + words_b);
  M->idx[0] = (int32_t*)(p + 2 * words_b);
  M->idx[1] = (int32_t*)(p + 2 * words_b + idx_b);
  return p + 2 * words_b + 2 * idx_b;
}

// rows: entries of each pair buffer; cnt: entries of each of the two counter arrays (0: none).
static int sort_mem(qe_ctx* ctx, Blocks& blk, int64_t rows, int64_t cnt, SortMem* M) {
  const size_t cnt_b = align256((size_t)cnt * 8);
  char* base;
  QE_TRY(blk.alloc(SORT_HEAD + SORT_HIST_B + pairs_bytes(rows) + 2 * cnt_b, (void**)&base));
  M->base = base;
  M->err = (unsigned*)base;
  M->hist = (uint32_t*)(base + SORT_HEAD);
  M->counts = (int64_t*)carve_pairs(base + SORT_HEAD + SORT_HIST_B, rows, M);
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
    hipLaunchKernelGGL(k_utf8_max_len, dim3(stride_grid(ctx, n)), dim3(256), 0, ctx->stream, keys[q].offsets, n,
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
  const int egrid = stride_grid(ctx, m, ENC_THREADS);
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
    for (int j = 0; j < nd; ++j, cur ^= 1)
      QE_TRY(sort_digit_pass(ctx, M.words[cur], M.idx[cur], j + 1 < nd ? M.words[cur ^ 1] : nullptr, M.idx[cur ^ 1], m,
                             8 * digits[j], M.counts, M.offs));
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
  Blocks blk(ctx);
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
static int topk_mem_pairs(Blocks& blk, int64_t rows, SortMem* M) {
  char* p;
  QE_TRY(blk.alloc(pairs_bytes(rows), (void**)&p));
  carve_pairs(p, rows, M);
  return QE_OK;
}

// The 8 digit histograms of word kw over the tied rows of the `cand` candidates in M.idx[cur] /
// M.words[cur] (implicit: over all n rows, and nothing else is written), read back.
static int topk_histogram(qe_ctx* ctx, const SortDesc& D, int64_t kw, int64_t n, bool implicit, int64_t cand, SortMem& M,
                          int cur) {
  const int egrid = stride_grid(ctx, cand, ENC_THREADS);
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
  Blocks blk(ctx);
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
    if (implicit) QE_TRY(topk_mem_pairs(blk, C.candidates(), &M));
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
  if (implicit) QE_TRY(topk_mem_pairs(blk, n, &M));  // no step ran: the candidates are all n rows
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
