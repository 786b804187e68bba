// Equi-join (build-defined operator): a device hash table built from one side's
// key column, probed by batches of the other, emitting (probe row, build row) index pairs in one
// fixed order: by probe row, and within a probe row by ascending build row.
//
// Table (qe_join_plan.hpp): open addressing, linear probing, 16-byte slots {key word, run start |
// run length << 32}; `slots` probed slots and the side slot `slots` for the key word that marks a
// free slot. rows[] holds the build row indices, every key's run contiguous and ascending.
//
// qe_join_build
//   k_join_valid  : non-null rows (nullable keys only; one read-back sizes the table)
//   k_join_insert : one row per lane: CAS the key word into its slot, count the slot's rows, keep
//                   the row's slot
//   exclusive scan of the slot counts -> run starts (slot order)
//   k_join_pack   : starts and counts into the slots; distinct keys and the longest run (read back)
//   longest run 1 : k_join_place, the slot holds its one build row itself (no rows[], no ordering)
//   otherwise     : rows[] = the row indices stably sorted by slot (the radix passes of qe_sort.hip),
//                   which is every run in slot order with its rows ascending
// qe_join_probe
//   k_join_count  : pairs per tile of JOIN_TILE probe rows, 8 rows per lane in flight
//   exclusive scan of the tile counts; the total is read back and checked against the capacity
//   k_join_emit   : looks the tile's rows up again, scans their counts inside the workgroup, and
//                   every lane writes its rows' runs
//   with QE_JOIN_TRACK, k_join_emit<true> also sets the mark of every slot whose run it writes
// qe_join_probe_mask
//   k_join_mask   : one row per lane, the BOOL words built per wave with __ballot; no host wait
// Match marks: one bit per slot of [0, slots] (the side slot included), allocated by the first call
// that sets one.
// qe_join_mark
//   k_join_mark   : one row per lane, the lookup of the probe and the marking of k_join_emit<true>
// qe_join_build_rows
//   k_join_flag_rows : one slot per lane: a marked slot stores 1 into the bytes of its run's rows
//                      (one working byte per build row, cleared first; a null-key row is in no run)
//   k_join_rows_count: rows per tile of JOIN_TILE build rows whose byte equals `matched`
//   exclusive scan of the tile counts; the total is read back and checked against the capacity
//   k_join_rows_emit : the tile's bytes again, scanned inside the workgroup; ascending row indices
#include "qe_rows.hpp"
#include "qe_join_plan.hpp"

#include <new>

struct qe_join {
  qe_ctx* ctx = nullptr;
  void* tab = nullptr;     // JSlot[slots + 1]
  int32_t* rows = nullptr; // build rows by run; NULL when every run has one row (or the table is empty)
  int64_t slots = 0, build_rows = 0, distinct = 0, max_dup = 0;
  int32_t type = 0;
  int64_t total_rows = 0;     // the build side's rows, null keys included
  uint32_t* marks = nullptr;  // join_mark_words(slots) words, from the first call that marks; else NULL
};

namespace qe {

struct JSlot {
  uint64_t key;
  uint64_t meta;  // run start (or, with runs of one row, the build row) | run length << 32
};

struct JKey {
  const void* values;
  const uint8_t* validity;
  int32_t type;
};

constexpr int JOIN_THREADS = 256;
constexpr int JOIN_TILE = JOIN_THREADS * 8;
// Build-time: the run length from which k_join_emit's wave writes a run together (0: a lane always
// walks its own run). A/B on the skewed and the mod-7 case: docs/experiments.md.
#ifndef QE_JOIN_COOP_MIN
#define QE_JOIN_COOP_MIN 32
#endif
constexpr int64_t JOIN_COOP_MIN = QE_JOIN_COOP_MIN;

// The key word of row i; false for a null row.
__device__ __forceinline__ bool join_row_word(const JKey& K, int64_t i, uint64_t* w) {
  if (!row_valid(K.validity, i)) return false;
  *w = join_key_word(K.type, load_fixed_raw(K.type, K.values, i));
  return true;
}

// The run of key word w: its slot's meta word, 0 when the key is absent. The table is at most
// half full, so a probe chain always ends at a free slot. SLOT: *slot = the slot of a hit (the side
// slot is S); without it the parameter compiles away.
template <bool SLOT = false>
__device__ __forceinline__ uint64_t join_lookup(const JSlot* __restrict__ tab, uint64_t S, uint64_t w,
                                                uint64_t* slot = nullptr) {
  if (w == JOIN_EMPTY_WORD) {
    if (SLOT) *slot = S;
    return tab[S].meta;
  }
  uint64_t s = join_home(w, S);
  for (;;) {
    const ulonglong2 e = *(const ulonglong2*)&tab[s];
    if (e.x == w) {
      if (SLOT) *slot = s;
      return e.y;
    }
    if (e.x == JOIN_EMPTY_WORD) return 0;
    s = (s + 1) & (S - 1);
  }
}

// Sets the mark of `slot`. The bit is read first and the atomic issued only when it is clear: a
// probe with millions of rows on one key costs reads, not atomics on one address. The read is a
// relaxed device-scope load, served by L2 where the atomics land; a plain load could keep meeting
// a line in this CU's L1 from before the bit was set. A stale read costs one redundant atomic.
__device__ __forceinline__ void join_set_mark(uint32_t* __restrict__ marks, uint64_t slot) {
  uint32_t* w = marks + join_mark_word(slot);
  const uint32_t b = join_mark_bit(slot);
  if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b)) atomicOr(w, b);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__global__ void __launch_bounds__(JOIN_THREADS) k_join_valid(const uint8_t* __restrict__ validity, int64_t n,
                                                             unsigned long long* __restrict__ out) {
  uint64_t c = 0;
  for (int64_t i = blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * JOIN_THREADS)
    c += row_valid(validity, i);
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// slotw[i] = the slot of build row i (S + 1 for a null row, which sorts behind every slot).
__global__ void __launch_bounds__(JOIN_THREADS) k_join_insert(JKey K, int64_t n, JSlot* __restrict__ tab, uint64_t S,
                                                              unsigned long long* __restrict__ cnt,
                                                              uint64_t* __restrict__ slotw) {
  for (int64_t i = blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * JOIN_THREADS) {
    uint64_t w, s = S + 1;
    if (join_row_word(K, i, &w)) {
      if (w == JOIN_EMPTY_WORD) {
        s = S;
      } else {
        s = join_home(w, S);
        for (;;) {
          unsigned long long k = *(volatile unsigned long long*)&tab[s].key;
          if (k == JOIN_EMPTY_WORD) k = atomicCAS((unsigned long long*)&tab[s].key, (unsigned long long)JOIN_EMPTY_WORD, (unsigned long long)w);
          if (k == JOIN_EMPTY_WORD || k == w) break;
          s = (s + 1) & (S - 1);
        }
      }
      atomicAdd(&cnt[s], 1ull);
    }
    slotw[i] = s;
  }
}

// Slot s of [0, S]: its run's start and length; stats[1] += keys, stats[2] = the longest run.
__global__ void __launch_bounds__(JOIN_THREADS) k_join_pack(JSlot* __restrict__ tab, const int64_t* __restrict__ cnt,
                                                            const int64_t* __restrict__ start, uint64_t S,
                                                            unsigned long long* __restrict__ stats) {
  uint64_t keys = 0, longest = 0;
  for (uint64_t s = blockIdx.x * (uint64_t)JOIN_THREADS + threadIdx.x; s <= S; s += (uint64_t)gridDim.x * JOIN_THREADS) {
    const uint64_t c = (uint64_t)cnt[s];
    tab[s].meta = (uint64_t)(uint32_t)start[s] | (c << 32);
    keys += c != 0;
    longest = c > longest ? c : longest;
  }
  keys = wave_sum(keys);
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t y = __shfl_xor(longest, off);
    longest = y > longest ? y : longest;
  }
  if ((threadIdx.x & 63) == 0) {
    if (keys) atomicAdd(&stats[1], (unsigned long long)keys);
    if (longest) atomicMax(&stats[2], (unsigned long long)longest);
  }
}

// Every run has one row: the slot holds the row itself.
__global__ void __launch_bounds__(JOIN_THREADS) k_join_place(const uint64_t* __restrict__ slotw, int64_t n,
                                                             JSlot* __restrict__ tab, uint64_t S) {
  for (int64_t i = blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * JOIN_THREADS) {
    const uint64_t s = slotw[i];
    if (s <= S) tab[s].meta = (uint64_t)(uint32_t)i | (1ull << 32);
  }
}

__global__ void __launch_bounds__(JOIN_THREADS) k_join_iota(int32_t* __restrict__ idx, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * JOIN_THREADS)
    idx[i] = (int32_t)i;
}

// Pairs of probe row i: its run's meta word (0: no match or a null key) and the pairs it emits.
// SLOT: *slot = the run's slot (set only when there is a run).
template <bool SLOT = false>
__device__ __forceinline__ uint64_t probe_row(const JKey& K, int64_t i, const JSlot* __restrict__ tab, uint64_t S,
                                              bool left, int64_t* pairs, uint64_t* slot = nullptr) {
  uint64_t w, m = 0;
  if (join_row_word(K, i, &w)) m = join_lookup<SLOT>(tab, S, w, slot);
  const int64_t c = (int64_t)(m >> 32);
  *pairs = left && c == 0 ? 1 : c;
  return m;
}

__global__ void __launch_bounds__(JOIN_THREADS) k_join_count(JKey K, int64_t n, const JSlot* __restrict__ tab, uint64_t S,
                                                             int left, int64_t* __restrict__ tcount) {
  __shared__ int64_t ws[JOIN_THREADS / 64];
  const int64_t g0 = (int64_t)blockIdx.x * JOIN_TILE;
  int64_t t = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = tile_elem(g0, k);
    int64_t c = 0;
    if (i < n) (void)probe_row(K, i, tab, S, left != 0, &c);
    t += c;
  }
  t = (int64_t)wave_sum((uint64_t)t);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t all = 0;
    for (int w = 0; w < JOIN_THREADS / 64; ++w) all += ws[w];
    tcount[blockIdx.x] = all;
  }
}

// toffs[tile] = pairs of the earlier tiles; `total` = all pairs (the capacity was checked against it).
// TRACK: every row that writes a run also marks the run's slot in `marks`, once per run; the
// untracked instantiation takes no part of it (`marks` is then NULL and unused).
template <bool TRACK>
__global__ void __launch_bounds__(JOIN_THREADS) k_join_emit(JKey K, int64_t n, const JSlot* __restrict__ tab, uint64_t S,
                                                            const int32_t* __restrict__ rows, int left,
                                                            const int64_t* __restrict__ toffs, int64_t total,
                                                            int32_t* __restrict__ probe_idx, int32_t* __restrict__ build_idx,
                                                            uint32_t* __restrict__ marks) {
  __shared__ int64_t ws[JOIN_THREADS / 64];
  const int64_t g0 = (int64_t)blockIdx.x * JOIN_TILE;
  int64_t v[8], ex[8];
  uint64_t m[8];
  uint64_t sl[TRACK ? 8 : 1];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t i = tile_elem(g0, k);
    v[k] = 0;
    m[k] = 0;
    if (TRACK) sl[TRACK ? k : 0] = 0;
    if (i < n) m[k] = probe_row<TRACK>(K, i, tab, S, left != 0, &v[k], TRACK ? &sl[TRACK ? k : 0] : nullptr);
  }
  (void)tile_excl<int64_t, JOIN_THREADS / 64>(v, ex, ws);
  const int64_t base = toffs[blockIdx.x];
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // (no lane leaves the loop early: the wave expands long runs together)
    const int64_t i = tile_elem(g0, k);
    const int64_t o = base + ex[k];
    const bool ok = v[k] != 0 && o >= 0 && o + v[k] <= total;  // (the second pass counts what the first did)
    const int64_t c = (int64_t)(m[k] >> 32);
    const int64_t st = (int64_t)(uint32_t)m[k];
    // a run of JOIN_COOP_MIN rows or more is written by the whole wave, 64 consecutive pairs per step
    const bool coop = JOIN_COOP_MIN > 0 && ok && rows && c >= JOIN_COOP_MIN;
    // (before the wave's runs: a lane whose run the wave writes leaves this step right after them)
    if (TRACK && ok && c > 0) join_set_mark(marks, sl[TRACK ? k : 0]);
    for (uint64_t big = __ballot(coop); big; big &= big - 1) {
      const int src = __builtin_ctzll(big);
      const int64_t oo = __shfl(o, src), cc = __shfl(c, src), ss = __shfl(st, src);
      const int32_t ii = (int32_t)__shfl(i, src);
      for (int64_t j = lane; j < cc; j += 64) {
        probe_idx[oo + j] = ii;
        build_idx[oo + j] = rows[ss + j];
      }
    }
    if (!ok || coop) continue;
    if (c == 0) {  // LEFT: the unmatched row's one pair
      probe_idx[o] = (int32_t)i;
      build_idx[o] = -1;
    } else if (!rows) {
      probe_idx[o] = (int32_t)i;
      build_idx[o] = (int32_t)st;
    } else {
      for (int64_t j = 0; j < c; ++j) {
        probe_idx[o + j] = (int32_t)i;
        build_idx[o + j] = rows[st + j];
      }
    }
  }
}

// mask bit i = (row i has a match) != anti; whole 32-bit words.
__global__ void __launch_bounds__(JOIN_THREADS) k_join_mask(JKey K, int64_t n, const JSlot* __restrict__ tab, uint64_t S,
                                                            int anti, uint32_t* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6, nwords = (n + 31) >> 5;
  const int64_t wave = (blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * JOIN_THREADS) >> 6;
  for (int64_t c = wave; c < nchunks; c += nwaves) {  // the same trip count in every lane of a wave
    const int64_t i = c * 64 + lane;
    bool b = false;
    if (i < n) {
      int64_t pairs;
      b = ((probe_row(K, i, tab, S, false, &pairs) >> 32) != 0) != (anti != 0);
    }
    store_bits64(mask, c, nwords, __ballot(b), lane);
  }
}

// The marking of a tracked probe alone: every row with a run marks the run's slot.
__global__ void __launch_bounds__(JOIN_THREADS) k_join_mark(JKey K, int64_t n, const JSlot* __restrict__ tab, uint64_t S,
                                                            uint32_t* __restrict__ marks) {
  for (int64_t i = blockIdx.x * (int64_t)JOIN_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * JOIN_THREADS) {
    int64_t pairs;
    uint64_t slot = 0;
    if (probe_row<true>(K, i, tab, S, false, &pairs, &slot) >> 32) join_set_mark(marks, slot);
  }
}

// flag[r] = 1 for every build row r of a marked slot's run (flag[] was cleared: a row of an unmarked
// key, and a null-key row, which is in no run, keep 0). One slot of [0, S] per lane; a run of
// JOIN_COOP_MIN rows or more is flagged by the whole wave, as k_join_emit writes one. Every row is
// in at most one run, so the byte stores never meet.
__global__ void __launch_bounds__(JOIN_THREADS) k_join_flag_rows(const JSlot* __restrict__ tab, uint64_t S,
                                                                 const int32_t* __restrict__ rows, int64_t nn, int64_t n,
                                                                 const uint32_t* __restrict__ marks,
                                                                 uint8_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const uint64_t nchunks = (S + 1 + 63) >> 6;
  const uint64_t wave = (blockIdx.x * (uint64_t)JOIN_THREADS + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * JOIN_THREADS) >> 6;
  for (uint64_t ch = wave; ch < nchunks; ch += nwaves) {  // the same trip count in every lane of a wave
    const uint64_t s = ch * 64 + lane;
    uint64_t m = 0;
    if (s <= S && (marks[join_mark_word(s)] & join_mark_bit(s))) m = tab[s].meta;
    const int64_t c = (int64_t)(m >> 32);
    const int64_t st = (int64_t)(uint32_t)m;
    if (!rows) {  // every run has one row: the slot holds it
      if (c != 0 && st < n) flag[st] = 1;
      continue;
    }
    const bool ok = c != 0 && st + c <= nn;  // (a run lies inside rows[], one entry per non-null row)
    const bool coop = JOIN_COOP_MIN > 0 && ok && c >= JOIN_COOP_MIN;
    for (uint64_t big = __ballot(coop); big; big &= big - 1) {
      const int src = __builtin_ctzll(big);
      const int64_t cc = __shfl(c, src), ss = __shfl(st, src);
      for (int64_t j = lane; j < cc; j += 64) {
        const int64_t r = rows[ss + j];
        if (r >= 0 && r < n) flag[r] = 1;
      }
    }
    if (!ok || coop) continue;
    for (int64_t j = 0; j < c; ++j) {
      const int64_t r = rows[st + j];
      if (r >= 0 && r < n) flag[r] = 1;
    }
  }
}

// This thread's 8 flag bytes of the tile at g0 as 0 / 1 answers "row i < n has flag == want"; flag[]
// is padded to whole 8-byte words.
__device__ __forceinline__ void rows_tile(const uint8_t* __restrict__ flag, int64_t g0, int64_t n, uint32_t want,
                                          int32_t (&v)[8]) {
  const int64_t e0 = tile_elem(g0, 0);
  const uint64_t f = e0 < n ? *(const uint64_t*)(flag + e0) : 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = e0 + k < n && (uint32_t)((f >> (8 * k)) & 0xFF) == want;
}

__global__ void __launch_bounds__(JOIN_THREADS) k_join_rows_count(const uint8_t* __restrict__ flag, int64_t n, uint32_t want,
                                                                  int64_t* __restrict__ tcount) {
  __shared__ int64_t ws[JOIN_THREADS / 64];
  int32_t v[8];
  rows_tile(flag, (int64_t)blockIdx.x * JOIN_TILE, n, want, v);
  uint64_t t = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) t += (uint64_t)v[k];
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = (int64_t)t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t all = 0;
    for (int w = 0; w < JOIN_THREADS / 64; ++w) all += ws[w];
    tcount[blockIdx.x] = all;
  }
}

// toffs[tile] = rows of the earlier tiles; `total` = all rows (the capacity was checked against it).
__global__ void __launch_bounds__(JOIN_THREADS) k_join_rows_emit(const uint8_t* __restrict__ flag, int64_t n, uint32_t want,
                                                                 const int64_t* __restrict__ toffs, int64_t total,
                                                                 int32_t* __restrict__ idx) {
  __shared__ int32_t ws[JOIN_THREADS / 64];
  const int64_t g0 = (int64_t)blockIdx.x * JOIN_TILE;
  int32_t v[8], ex[8];
  rows_tile(flag, g0, n, want, v);
  (void)tile_excl<int32_t, JOIN_THREADS / 64>(v, ex, ws);
  const int64_t base = toffs[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t o = base + ex[k];
    if (v[k] && o >= 0 && o < total) idx[o] = (int32_t)tile_elem(g0, k);  // (the second pass counts what the first did)
  }
}

namespace {

int check_key(const char* what, const qe_column* key) {
  QE_CHECK(key != nullptr, QE_ERR_INVALID_ARG, "%s: null key column", what);
  QE_CHECK(join_key_type(key->type), QE_ERR_INVALID_ARG,
           "%s: key type %d (one INT64, INT32, DATE32, UINT8, BOOL or FLOAT64 column)", what, key->type);
  QE_CHECK(key->length >= 0 && key->length <= JOIN_MAX_ROWS, QE_ERR_INVALID_ARG, "%s: %lld key rows (at most 2^31 - 1)", what,
           (long long)key->length);
  QE_CHECK(key->values || key->length == 0, QE_ERR_INVALID_ARG, "%s: the key column has no values", what);
  return QE_OK;
}

int check_probe(const char* what, const qe_join* j, const qe_column* key) {
  QE_CHECK(j != nullptr && j->ctx != nullptr, QE_ERR_INVALID_ARG, "%s: null join", what);
  QE_TRY(ctx_enter(j->ctx));
  QE_TRY(check_key(what, key));
  QE_CHECK(join_compatible(j->type, key->type), QE_ERR_INVALID_ARG,
           "%s: a probe key of type %d does not join a build key of type %d (FLOAT64 joins only FLOAT64)", what, key->type,
           j->type);
  return QE_OK;
}

// The mark bitmap, allocated and cleared (stream-ordered) by the first call that marks.
int ensure_marks(qe_join* j) {
  if (j->marks) return QE_OK;
  const size_t bytes = (size_t)join_mark_words(j->slots) * 4;
  Blocks blk(j->ctx);
  void* p;
  QE_TRY(blk.alloc(bytes, &p));
  QE_HIP(hipMemsetAsync(p, 0, bytes, j->ctx->stream));
  blk.keep(p);
  j->marks = (uint32_t*)p;
  return QE_OK;
}

}  // namespace

}  // namespace qe

using namespace qe;

extern "C" {

int qe_join_build(qe_ctx* ctx, const qe_column* key, qe_join** out) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(out != nullptr, QE_ERR_INVALID_ARG, "join build: null output");
  *out = nullptr;
  QE_TRY(check_key("join build", key));
  const int64_t n = key->length;
  const JKey K{key->values, key->validity, key->type};
  Blocks blk(ctx);
  void* hp;
  QE_TRY(ctx_pinned(ctx, 32, &hp));
  const unsigned long long* h_stats = (const unsigned long long*)hp;
  unsigned long long* d_stats;  // [0] non-null rows, [1] distinct keys, [2] the longest run
  QE_TRY(blk.alloc(32, (void**)&d_stats));
  QE_HIP(hipMemsetAsync(d_stats, 0, 32, ctx->stream));

  int64_t nn = n;
  if (key->validity && n > 0) {
    hipLaunchKernelGGL(k_join_valid, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, key->validity, n, d_stats);
    QE_TRY(launch_check("k_join_valid"));
    QE_HIP(hipMemcpyAsync(hp, d_stats, 32, hipMemcpyDeviceToHost, ctx->stream));
    QE_TRY(ctx_sync(ctx));
    nn = (int64_t)h_stats[0];
  }
  const int64_t S = join_slots(nn);
  JSlot* tab;
  int64_t *cnt, *start;
  uint64_t* slotw;
  QE_TRY(blk.alloc((size_t)(S + 1) * sizeof(JSlot), (void**)&tab));
  QE_TRY(blk.alloc((size_t)(S + 1) * 8, (void**)&cnt));
  QE_TRY(blk.alloc((size_t)(S + 2) * 8, (void**)&start));
  QE_TRY(blk.alloc((size_t)n * 8, (void**)&slotw));
  QE_HIP(hipMemsetAsync(tab, 0xFF, (size_t)(S + 1) * sizeof(JSlot), ctx->stream));
  QE_HIP(hipMemsetAsync(cnt, 0, (size_t)(S + 1) * 8, ctx->stream));
  if (n > 0) {
    hipLaunchKernelGGL(k_join_insert, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, K, n, tab, (uint64_t)S,
                       (unsigned long long*)cnt, slotw);
    QE_TRY(launch_check("k_join_insert"));
  }
  QE_TRY(exclusive_scan_i64(ctx, cnt, start, S + 1));
  hipLaunchKernelGGL(k_join_pack, dim3(stride_grid(ctx, S + 1)), dim3(JOIN_THREADS), 0, ctx->stream, tab, cnt, start,
                     (uint64_t)S, d_stats);
  QE_TRY(launch_check("k_join_pack"));
  QE_HIP(hipMemcpyAsync(hp, d_stats, 32, hipMemcpyDeviceToHost, ctx->stream));
  QE_TRY(ctx_sync(ctx));  // the longest run decides whether the rows need ordering, and sizes it
  const int64_t distinct = (int64_t)h_stats[1], max_dup = (int64_t)h_stats[2];

  int32_t* rows = nullptr;
  if (max_dup == 1) {
    hipLaunchKernelGGL(k_join_place, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, slotw, n, tab, (uint64_t)S);
    QE_TRY(launch_check("k_join_place"));
  } else if (max_dup > 1) {
    uint64_t* words[2] = {slotw, nullptr};
    int32_t* idx[2] = {nullptr, nullptr};
    void* scratch;
    QE_TRY(blk.alloc((size_t)n * 8, (void**)&words[1]));
    QE_TRY(blk.alloc((size_t)n * 4, (void**)&idx[0]));
    QE_TRY(blk.alloc((size_t)n * 4, (void**)&idx[1]));
    QE_TRY(blk.alloc(sort_pairs_scratch_bytes(n), &scratch));
    QE_TRY(blk.alloc((size_t)nn * 4, (void**)&rows));
    hipLaunchKernelGGL(k_join_iota, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, idx[0], n);
    QE_TRY(launch_check("k_join_iota"));
    int bits = 1;
    while (((uint64_t)S + 1) >> bits) ++bits;  // slot words reach S + 1
    int cur = 0;
    QE_TRY(sort_pairs(ctx, words, idx, n, bits, scratch, &cur));
    // the null rows sorted last: the first nn indices are the runs in slot order
    QE_HIP(hipMemcpyAsync(rows, idx[cur], (size_t)nn * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }

  qe_join* j = new (std::nothrow) qe_join();
  QE_CHECK(j != nullptr, QE_ERR_OOM, "join build: out of host memory");
  j->ctx = ctx;
  j->tab = tab;
  j->rows = rows;
  j->slots = S;
  j->build_rows = nn;
  j->total_rows = n;
  j->distinct = distinct;
  j->max_dup = max_dup;
  j->type = key->type;
  blk.keep(tab);
  if (rows) blk.keep(rows);
  *out = j;
  return QE_OK;
}

int qe_join_destroy(qe_join* j) {
  if (!j) return QE_OK;
  if (j->ctx) {
    dev_free(j->ctx, j->tab);
    dev_free(j->ctx, j->rows);
    dev_free(j->ctx, j->marks);
  }
  delete j;
  return QE_OK;
}

int qe_join_stats(qe_join* j, int64_t* build_rows, int64_t* distinct, int64_t* max_dup, int64_t* slots) {
  QE_CHECK(j != nullptr && j->ctx != nullptr, QE_ERR_INVALID_ARG, "join stats: null join");
  QE_TRY(ctx_enter(j->ctx));
  QE_TRY(ctx_sync(j->ctx));
  if (build_rows) *build_rows = j->build_rows;
  if (distinct) *distinct = j->distinct;
  if (max_dup) *max_dup = j->max_dup;
  if (slots) *slots = j->slots;
  return QE_OK;
}

int qe_join_probe(qe_join* j, const qe_column* key, int32_t kind, qe_column* probe_idx, qe_column* build_idx,
                  int64_t* pairs) {
  QE_TRY(check_probe("join probe", j, key));
  qe_ctx* ctx = j->ctx;
  int32_t base;
  bool track;
  QE_CHECK(join_probe_kind(kind, &base, &track), QE_ERR_INVALID_ARG, "join probe: kind %d", kind);
  const int left = base == QE_JOIN_LEFT ? 1 : 0;
  QE_CHECK(probe_idx && build_idx && pairs, QE_ERR_INVALID_ARG, "join probe: null output");
  QE_CHECK(probe_idx->type == QE_TYPE_INT32 && !probe_idx->validity && build_idx->type == QE_TYPE_INT32 && !build_idx->validity,
           QE_ERR_INVALID_ARG, "join probe: the index columns must be INT32 without validity");
  const int64_t n = key->length;
  const int64_t cap = std::min(probe_idx->length, build_idx->length);
  *pairs = 0;
  if (n == 0) {
    QE_CHECK(cap >= 0, QE_ERR_INVALID_ARG, "join probe: negative capacity");
    probe_idx->length = build_idx->length = 0;
    return QE_OK;
  }
  const JKey K{key->values, key->validity, key->type};
  const int64_t ntiles = (int64_t)div_up((uint64_t)n, JOIN_TILE);
  Blocks blk(ctx);
  int64_t *tcount, *toffs;
  QE_TRY(blk.alloc((size_t)ntiles * 8, (void**)&tcount));
  QE_TRY(blk.alloc((size_t)(ntiles + 1) * 8, (void**)&toffs));
  hipLaunchKernelGGL(k_join_count, dim3((unsigned)ntiles), dim3(JOIN_THREADS), 0, ctx->stream, K, n, (const JSlot*)j->tab,
                     (uint64_t)j->slots, left, tcount);
  QE_TRY(launch_check("k_join_count"));
  QE_TRY(exclusive_scan_i64(ctx, tcount, toffs, ntiles));
  void* hp;
  QE_TRY(ctx_pinned(ctx, 8, &hp));
  QE_HIP(hipMemcpyAsync(hp, toffs + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  QE_TRY(ctx_sync(ctx));
  const int64_t total = *(const int64_t*)hp;
  *pairs = total;
  QE_CHECK(total <= JOIN_MAX_ROWS, QE_ERR_UNSUPPORTED, "join probe: %lld pairs (at most 2^31 - 1 per call)", (long long)total);
  QE_CHECK(total <= cap, QE_ERR_CAPACITY, "join probe: the index columns hold %lld rows, need %lld", (long long)cap,
           (long long)total);
  QE_CHECK(total == 0 || (probe_idx->values && build_idx->values), QE_ERR_INVALID_ARG, "join probe: an index column has no values");
  if (total > 0) {  // (no pair, no match: nothing to mark either)
    // marking is the emit pass's: a call refused above has left the marks alone
    if (track) QE_TRY(ensure_marks(j));
    hipLaunchKernelGGL(track ? k_join_emit<true> : k_join_emit<false>, dim3((unsigned)ntiles), dim3(JOIN_THREADS), 0,
                       ctx->stream, K, n, (const JSlot*)j->tab, (uint64_t)j->slots, (const int32_t*)j->rows, left,
                       (const int64_t*)toffs, total, (int32_t*)probe_idx->values, (int32_t*)build_idx->values,
                       track ? j->marks : (uint32_t*)nullptr);
    QE_TRY(launch_check("k_join_emit"));
  }
  probe_idx->length = build_idx->length = total;
  return QE_OK;
}

int qe_join_probe_mask(qe_join* j, const qe_column* key, int32_t anti, qe_column* mask) {
  QE_TRY(check_probe("join probe mask", j, key));
  qe_ctx* ctx = j->ctx;
  QE_CHECK(mask != nullptr && mask->type == QE_TYPE_BOOL && !mask->validity, QE_ERR_INVALID_ARG,
           "join probe mask: the mask must be a BOOL column without validity");
  const int64_t n = key->length;
  QE_CHECK(mask->length >= n, QE_ERR_CAPACITY, "join probe mask: the mask holds %lld rows, need %lld", (long long)mask->length,
           (long long)n);
  QE_CHECK(n == 0 || (mask->values && ((uintptr_t)mask->values & 3) == 0), QE_ERR_INVALID_ARG,
           "join probe mask: the mask needs a 4-byte aligned values buffer");
  mask->length = n;
  if (n == 0) return QE_OK;
  const JKey K{key->values, key->validity, key->type};
  hipLaunchKernelGGL(k_join_mask, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, K, n, (const JSlot*)j->tab,
                     (uint64_t)j->slots, anti ? 1 : 0, (uint32_t*)mask->values);
  return launch_check("k_join_mask");
}

int qe_join_mark(qe_join* j, const qe_column* key) {
  QE_TRY(check_probe("join mark", j, key));
  qe_ctx* ctx = j->ctx;
  const int64_t n = key->length;
  if (n == 0) return QE_OK;
  QE_TRY(ensure_marks(j));
  const JKey K{key->values, key->validity, key->type};
  hipLaunchKernelGGL(k_join_mark, dim3(stride_grid(ctx, n)), dim3(JOIN_THREADS), 0, ctx->stream, K, n, (const JSlot*)j->tab,
                     (uint64_t)j->slots, j->marks);
  return launch_check("k_join_mark");
}

int qe_join_clear_marks(qe_join* j) {
  QE_CHECK(j != nullptr && j->ctx != nullptr, QE_ERR_INVALID_ARG, "join clear marks: null join");
  QE_TRY(ctx_enter(j->ctx));
  if (j->marks) QE_HIP(hipMemsetAsync(j->marks, 0, (size_t)join_mark_words(j->slots) * 4, j->ctx->stream));
  return QE_OK;
}

int qe_join_build_rows(qe_join* j, int32_t matched, qe_column* idx, int64_t* rows) {
  QE_CHECK(j != nullptr && j->ctx != nullptr, QE_ERR_INVALID_ARG, "join build rows: null join");
  qe_ctx* ctx = j->ctx;
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(idx && rows, QE_ERR_INVALID_ARG, "join build rows: null output");
  QE_CHECK(idx->type == QE_TYPE_INT32 && !idx->validity, QE_ERR_INVALID_ARG,
           "join build rows: the index column must be INT32 without validity");
  const int64_t cap = idx->length;
  QE_CHECK(cap >= 0, QE_ERR_INVALID_ARG, "join build rows: negative capacity");
  const int64_t n = j->total_rows;
  *rows = 0;
  if (n == 0) {
    idx->length = 0;
    return QE_OK;
  }
  const int64_t ntiles = (int64_t)div_up((uint64_t)n, JOIN_TILE);
  const size_t fbytes = ((size_t)n + 7) & ~(size_t)7;  // k_join_rows_* read whole 8-byte words
  Blocks blk(ctx);
  uint8_t* flag;
  int64_t *tcount, *toffs;
  QE_TRY(blk.alloc(fbytes, (void**)&flag));
  QE_TRY(blk.alloc((size_t)ntiles * 8, (void**)&tcount));
  QE_TRY(blk.alloc((size_t)(ntiles + 1) * 8, (void**)&toffs));
  QE_HIP(hipMemsetAsync(flag, 0, fbytes, ctx->stream));
  if (j->marks && j->build_rows > 0) {  // (never tracked: every mark is clear, every row unmatched)
    hipLaunchKernelGGL(k_join_flag_rows, dim3(stride_grid(ctx, j->slots + 1)), dim3(JOIN_THREADS), 0, ctx->stream,
                       (const JSlot*)j->tab, (uint64_t)j->slots, (const int32_t*)j->rows, j->build_rows, n,
                       (const uint32_t*)j->marks, flag);
    QE_TRY(launch_check("k_join_flag_rows"));
  }
  const uint32_t want = matched ? 1u : 0u;
  hipLaunchKernelGGL(k_join_rows_count, dim3((unsigned)ntiles), dim3(JOIN_THREADS), 0, ctx->stream, (const uint8_t*)flag, n,
                     want, tcount);
  QE_TRY(launch_check("k_join_rows_count"));
  QE_TRY(exclusive_scan_i64(ctx, tcount, toffs, ntiles));
  void* hp;
  QE_TRY(ctx_pinned(ctx, 8, &hp));
  QE_HIP(hipMemcpyAsync(hp, toffs + ntiles, 8, hipMemcpyDeviceToHost, ctx->stream));
  QE_TRY(ctx_sync(ctx));
  const int64_t total = *(const int64_t*)hp;
  *rows = total;
  QE_CHECK(total <= cap, QE_ERR_CAPACITY, "join build rows: the index column holds %lld rows, need %lld", (long long)cap,
           (long long)total);
  QE_CHECK(total == 0 || idx->values, QE_ERR_INVALID_ARG, "join build rows: the index column has no values");
  if (total > 0) {
    hipLaunchKernelGGL(k_join_rows_emit, dim3((unsigned)ntiles), dim3(JOIN_THREADS), 0, ctx->stream, (const uint8_t*)flag, n,
                       want, (const int64_t*)toffs, total, (int32_t*)idx->values);
    QE_TRY(launch_check("k_join_rows_emit"));
  }
  idx->length = total;
  return QE_OK;
}

}  // extern "C"
