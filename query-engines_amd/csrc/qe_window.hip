// Window functions: qe_window_boundaries, qe_window_eval, qe_window_eval_frames,
// qe_window_layout.
//
// Everything works on SORTED POSITIONS i = 0 .. n-1 of the permutation `order` (row order[i] stands
// at position i) until the last step, which runs one lane per INPUT ROW through the inverse
// permutation and writes the results at the input's row positions.
//
//   boundaries : one lane per position compares rows order[i-1] and order[i] on every key; a wave's
//                64 answers become two bitmap words (__ballot).
//   scans      : every index a function needs comes from a scan, and all scans of a call share one
//                machinery (WinJob). Over the WORDS of the two boundary bitmaps (n / 32 elements): the
//                last set bit at or before each word (max) and the first at or after it (min, scanned
//                from the right), which with one clz / ffs in the row's own word give the partition
//                and peer group's first and last positions, and the peer bitmap's running popcount
//                (DENSE_RANK). Over the POSITIONS: the running (wrapping int64 sum, non-null count) of
//                a gathered input (SUM and COUNT(x) of a frame [P, e] are S[e] - S[P-1], exact modulo
//                2^64, so this scan is not segmented), and the segmented MIN / MAX scan whose element
//                carries (best non-NaN value, has a value, the first value is NaN, has a non-NaN
//                value) and keeps the window-earlier operand on ties. MIN / MAX over a bounded frame
//                (ROWS BETWEEN lo AND hi, at most L = hi - lo + 1 rows) reads two such scans that also
//                restart at every block of L positions, one from the left and one from the right: a
//                frame straddles at most one block edge, so it is the backward scan at its first
//                position combined with the forward scan at its last, whatever L is.
//                A tile is WIN_THREADS x WIN_ITEMS consecutive elements; carries cross tiles by tile
//                reduce -> one workgroup scanning the tile aggregates -> apply (no look-back, nothing
//                spins).
//   evaluate   : one lane per POSITION computes every function into a staging record (the values,
//                then their validity bits), reading the scans where neighbouring lanes read them; then
//                one lane per INPUT ROW r copies the record of position inv[r] to the outputs, values
//                coalesced and validity by __ballot, so a row costs one scattered record read
//                whatever the number of functions. The records cross LDS both ways (win_eval_block,
//                win_emit_block). (Evaluating per input row, with every scan read scattered,
//                measured 26.7 ms for eight functions over 100M rows.)
// n <= WIN_SMALL_MAX runs all of it as ONE launch of one workgroup that walks its tiles in turn.
//
// An `order` entry outside [0, n) is never used as an index: its position gathers a null, the inverse
// permutation keeps -1 for the rows no position names (their results are null / 0), and a device flag
// fails the call.
#include "qe_rows.hpp"
#include "qe_window_plan.hpp"

namespace qe {
namespace {

struct WinElem {  // one scan element
  int64_t v;
  int32_t f;  // SUM scan: non-null count; MIN / MAX scan: WF_* flags
  int32_t pad;
};
static_assert(sizeof(WinElem) == WIN_ELEM_BYTES, "window_tile_bytes sizes the tile arrays by WIN_ELEM_BYTES");

enum { WS_PREV = 0, WS_NEXT, WS_POPC, WS_SUM, WS_MIN, WS_MAX };  // what a scan job scans
constexpr int32_t WF_HAS = 1, WF_SEEDNAN = 2, WF_HASNUM = 4, WF_RESET = 8;
constexpr int WIN_MAX_JOBS = WIN_WORD_SCANS + 2 * QE_MAX_AGGS;  // a bounded MIN / MAX reads two position scans
constexpr int WIN_WAVES = WIN_THREADS / 64;
constexpr int64_t WIN_CANON_NAN = 0x7FF8000000000000ll;

struct WinJob {
  int32_t src;      // WS_*
  int32_t in_type;  // position scans: the input column's type
  int32_t back;     // MIN / MAX scans: element k is position count - 1 - k (the scan runs from the right)
  uint32_t block;   // MIN / MAX scans: > 0 restarts the scan at every block of this many positions
  const uint32_t* bits;  // word scans: the bitmap
  const void* in;        // position scans: the input column
  const uint8_t* in_valid;
  int64_t count;    // elements: bitmap words, or positions
  int64_t* out_v;   // position scans: the scanned values
  int32_t* out_f;   // position scans: counts / flags; word scans: the scanned word values
};

struct WinCommon {
  const int32_t* order;
  const uint32_t* part;
  const uint32_t* peer;
  int64_t n, nw;
  int32_t* inv;
  unsigned* flag;
};

struct WinEvalFn {
  int32_t fn, frame, in_type, out_width;
  int64_t offset;
  int64_t lo, hi;  // QE_FRAME_ROWS_BETWEEN: the bounds, clamped to [-n, n]
  int64_t block;   // MIN / MAX: the block length of its scans (0: none)
  const void* in;
  const uint8_t* in_valid;
  const int64_t* scan_v;  // the forward scan (SUM / COUNT: the running pair)
  const int32_t* scan_f;
  const int64_t* back_v;  // MIN / MAX: the backward scan
  const int32_t* back_f;
  void* out;
  uint32_t* out_valid;
};

struct WinArgs {
  WinCommon c;
  int32_t njobs, nfns, need_dense, pad;
  const int32_t *prev_part, *next_part, *prev_peer, *next_peer, *cum_peer;
  WinElem* tile_agg;    // [job][tile]
  WinElem* tile_carry;  // [job][tile]: the scan of everything before the tile
  int64_t* stage;       // [position][nfns + 1]: every function's value, then the validity bits
  int64_t tile_stride;
  WinJob jobs[WIN_MAX_JOBS];
  WinEvalFn fns[QE_MAX_AGGS];
};
static_assert(sizeof(WinArgs) <= 4096, "WinArgs is passed by value: the kernel-argument segment holds 4 KiB");

// ---- bitmap words -----------------------------------------------------------------------------------
// Word w of a boundary bitmap as the scans read it: bits at and past n cleared, bit 0 of word 0 set
// (position 0 starts a run whatever the caller's buffer holds), so every index derived from the
// words lies in [0, n).
__device__ __forceinline__ uint32_t win_word(const uint32_t* __restrict__ bm, int64_t w, int64_t n) {
  uint32_t x = bm[w];
  const int64_t left = n - 32 * w;
  if (left < 32) x &= (1u << left) - 1u;
  if (w == 0) x |= 1u;
  return x;
}

// Row r of a fixed-width column as int64: integers by value, FLOAT64 its bits (0 for other types,
// whose values COUNT never reads).
__device__ __forceinline__ int64_t win_value(int32_t type, const void* __restrict__ in, int64_t r) {
  switch (type) {
    case QE_TYPE_INT64:
    case QE_TYPE_FLOAT64: return ((const int64_t*)in)[r];
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32: return ((const int32_t*)in)[r];
    case QE_TYPE_UINT8: return ((const uint8_t*)in)[r];
    default: return 0;
  }
}

__device__ __forceinline__ bool win_is_nan(int64_t bits) { return ((uint64_t)bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// ---- the scan operator ------------------------------------------------------------------------------
__device__ __forceinline__ WinElem win_identity(int32_t src) {
  WinElem e;
  e.v = src == WS_PREV ? -1 : src == WS_NEXT ? INT64_MAX : 0;
  e.f = 0;
  e.pad = 0;
  return e;
}

// MIN / MAX of the rows of l followed by the rows of h, l the earlier in WINDOW order (the flags
// without WF_RESET). Associative, not commutative: the first non-null value seeds the NaN, and of equal
// values the earlier stays.
__device__ __forceinline__ WinElem win_merge(bool is_max, int32_t in_type, const WinElem& l, const WinElem& h) {
  WinElem r;
  r.pad = 0;
  r.f = ((l.f | h.f) & (WF_HAS | WF_HASNUM)) | (((l.f & WF_HAS) ? l.f : h.f) & WF_SEEDNAN);
  if ((l.f & WF_HASNUM) && (h.f & WF_HASNUM)) {
    bool take_h;  // strictly better only: the earlier of equal values stays (-0.0 == +0.0)
    if (in_type == QE_TYPE_FLOAT64) {
      const double x = __longlong_as_double(l.v), y = __longlong_as_double(h.v);
      take_h = is_max ? y > x : y < x;
    } else {
      take_h = is_max ? h.v > l.v : h.v < l.v;
    }
    r.v = take_h ? h.v : l.v;
  } else {
    r.v = (l.f & WF_HASNUM) ? l.v : h.v;
  }
  return r;
}

// a then b in SCAN order (a covers the elements scanned earlier). Associative for every src; not
// commutative for MIN / MAX.
__device__ __forceinline__ WinElem win_combine(const WinJob& J, const WinElem& a, const WinElem& b) {
  WinElem r;
  r.pad = 0;
  switch (J.src) {
    case WS_PREV:
      r.v = a.v > b.v ? a.v : b.v;
      r.f = 0;
      return r;
    case WS_NEXT:
      r.v = a.v < b.v ? a.v : b.v;
      r.f = 0;
      return r;
    case WS_POPC:
    case WS_SUM:
      r.v = (int64_t)((uint64_t)a.v + (uint64_t)b.v);
      r.f = a.f + b.f;
      return r;
    default: break;
  }
  if (b.f & WF_RESET) return b;  // b starts a segment: nothing scanned before it counts
  // a backward scan meets the window-later rows first: b is then the window-earlier operand
  r = J.back ? win_merge(J.src == WS_MAX, J.in_type, b, a) : win_merge(J.src == WS_MAX, J.in_type, a, b);
  r.f |= a.f & WF_RESET;
  return r;
}

// Where element k (< count) of a position scan lives: its position.
__device__ __forceinline__ int64_t win_slot(const WinJob& J, int64_t k) { return J.back ? J.count - 1 - k : k; }

// Element k of a job (the identity past its count).
__device__ __forceinline__ WinElem win_load(const WinJob& J, const WinCommon& C, int64_t k) {
  WinElem e = win_identity(J.src);
  if (k >= J.count) return e;
  switch (J.src) {
    case WS_PREV: {
      const uint32_t x = win_word(J.bits, k, C.n);
      e.v = x ? 32 * k + 31 - __clz((int)x) : -1;
      return e;
    }
    case WS_NEXT: {  // scanned from the right: element k is word count - 1 - k
      const int64_t w = J.count - 1 - k;
      const uint32_t x = win_word(J.bits, w, C.n);
      e.v = x ? 32 * w + (__ffs((int)x) - 1) : C.n;
      return e;
    }
    case WS_POPC: e.v = __popc(win_word(J.bits, k, C.n)); return e;
    default: break;
  }
  const int64_t p = win_slot(J, k);
  const int64_t r = C.order[p];
  const bool valid = (uint64_t)r < (uint64_t)C.n && row_valid(J.in_valid, r);
  const int64_t v = valid ? win_value(J.in_type, J.in, r) : 0;
  if (J.src == WS_SUM) {
    e.v = v;
    e.f = valid ? 1 : 0;
    return e;
  }
  const bool nan = valid && J.in_type == QE_TYPE_FLOAT64 && win_is_nan(v);
  e.v = nan ? 0 : v;
  e.f = valid ? (WF_HAS | (nan ? WF_SEEDNAN : WF_HASNUM)) : 0;
  // a segment starts at a partition's first position and at a block's (backward: at their last)
  bool reset;
  if (!J.back) {
    reset = p == 0 || ((C.part[p >> 5] >> (p & 31)) & 1) || (J.block && (uint32_t)p % J.block == 0);
  } else {
    const int64_t q = p + 1;
    reset = q == C.n || ((C.part[q >> 5] >> (q & 31)) & 1) || (J.block && (uint32_t)q % J.block == 0);
  }
  if (reset) e.f |= WF_RESET;
  return e;
}

__device__ __forceinline__ void win_store(const WinJob& J, int64_t k, const WinElem& e) {
  if (k >= J.count) return;
  switch (J.src) {
    case WS_PREV:
    case WS_POPC: J.out_f[k] = (int32_t)e.v; break;
    case WS_NEXT: J.out_f[J.count - 1 - k] = (int32_t)e.v; break;
    default: {
      const int64_t p = win_slot(J, k);
      J.out_v[p] = e.v;
      J.out_f[p] = e.f;
    }
  }
}

// Inclusive scan of a workgroup's tile, thread t holding elements WIN_ITEMS t .. + WIN_ITEMS - 1, after
// `carry` (the scan of everything before the tile). Returns the tile's own aggregate (without the
// carry) to every thread. ws: WIN_WAVES elements of LDS. Every thread of the workgroup calls it.
__device__ __forceinline__ WinElem win_block_scan(const WinJob& J, WinElem (&x)[WIN_ITEMS], const WinElem& carry, WinElem* ws) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 1; j < WIN_ITEMS; ++j) x[j] = win_combine(J, x[j - 1], x[j]);
  WinElem t = x[WIN_ITEMS - 1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    WinElem y;
    y.v = __shfl_up((long long)t.v, off);
    y.f = __shfl_up(t.f, off);
    y.pad = 0;
    if (lane >= off) t = win_combine(J, y, t);
  }
  if (lane == 63) ws[wid] = t;
  __syncthreads();
  WinElem wp = win_identity(J.src), all = win_identity(J.src);
#pragma unroll
  for (int w = 0; w < WIN_WAVES; ++w) {
    const WinElem s = ws[w];
    if (w < wid) wp = win_combine(J, wp, s);
    all = win_combine(J, all, s);
  }
  __syncthreads();  // ws is rewritten by the next tile
  WinElem ex;
  ex.v = __shfl_up((long long)t.v, 1);
  ex.f = __shfl_up(t.f, 1);
  ex.pad = 0;
  if (lane == 0) ex = win_identity(J.src);
  const WinElem base = win_combine(J, carry, win_combine(J, wp, ex));
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) x[j] = win_combine(J, base, x[j]);
  return all;
}

// One tile of a job. WP_ONE: load, scan after `carry`, store (the one-workgroup path). The
// multi-workgroup passes gather a position scan's input only once: WP_REDUCE loads, leaves a
// position scan's elements as loaded in the job's output arrays, and scans for the tile's aggregate;
// WP_APPLY reads them back from there (a word scan loads its bitmap again), scans after the tile's
// carry and stores.
enum { WP_ONE = 0, WP_REDUCE, WP_APPLY };
__device__ __forceinline__ WinElem win_scan_tile(const WinJob& J, const WinCommon& C, int64_t tile, const WinElem& carry, int phase,
                                                 WinElem* ws) {
  WinElem x[WIN_ITEMS];
  const int64_t k0 = tile * WIN_TILE + (int64_t)threadIdx.x * WIN_ITEMS;
  const bool positions = J.src >= WS_SUM;
  if (phase == WP_APPLY && positions) {
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) {
      x[j] = win_identity(J.src);
      if (k0 + j < J.count) {
        const int64_t p = win_slot(J, k0 + j);
        x[j].v = J.out_v[p];
        x[j].f = J.out_f[p];
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) x[j] = win_load(J, C, k0 + j);
    if (phase == WP_REDUCE && positions) {
#pragma unroll
      for (int j = 0; j < WIN_ITEMS; ++j) win_store(J, k0 + j, x[j]);
    }
  }
  const WinElem all = win_block_scan(J, x, carry, ws);
  if (phase != WP_REDUCE) {
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) win_store(J, k0 + j, x[j]);
  }
  return all;
}

// ---- evaluate ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t win_mask_le(int64_t i) { return 0xFFFFFFFFu >> (31 - (int)(i & 31)); }

// Every function at sorted position i (i < n), into the record `rec`: A.nfns values, then one word of
// validity bits. Everything read here lies at or near i (the scans at the frame's
// ends, the bitmap words), but for LAG / LEAD's gather of the other row.
__device__ __forceinline__ void win_eval_pos(const WinArgs& A, int64_t i, int64_t* rec) {
  const WinCommon& C = A.c;
  const int64_t n = C.n;
  const int64_t wi = i >> 5;
  const uint32_t le = win_mask_le(i);
  const uint32_t pw = win_word(C.part, wi, n), gw = win_word(C.peer, wi, n);
  uint32_t m = pw & le;  // (word 0 always has bit 0: wi - 1 is read only for wi > 0)
  const int64_t P = m ? 32 * wi + 31 - __clz((int)m) : (int64_t)A.prev_part[wi - 1];
  m = gw & le;
  int64_t G = m ? 32 * wi + 31 - __clz((int)m) : (int64_t)A.prev_peer[wi - 1];
  if (G < P) G = P;
  m = pw & ~le;
  const int64_t Pe = (m ? 32 * wi + (__ffs((int)m) - 1) : (wi + 1 < C.nw ? (int64_t)A.next_part[wi + 1] : n)) - 1;
  m = gw & ~le;
  int64_t Ge = (m ? 32 * wi + (__ffs((int)m) - 1) : (wi + 1 < C.nw ? (int64_t)A.next_peer[wi + 1] : n)) - 1;
  if (Ge > Pe) Ge = Pe;
  int64_t dense = 1;
  if (A.need_dense) {  // peer starts in (P, i], plus the one at P
    const int64_t wp = P >> 5;
    const int64_t ri = (wi ? (int64_t)A.cum_peer[wi - 1] : 0) + __popc(gw & le);
    const int64_t rp = (wp ? (int64_t)A.cum_peer[wp - 1] : 0) + __popc(win_word(C.peer, wp, n) & win_mask_le(P));
    dense = ri - rp + 1;
  }
  uint64_t valid_bits = 0;
  for (int k = 0; k < A.nfns; ++k) {
    const WinEvalFn& F = A.fns[k];
    // the frame [s, e] (nothing is read at s or e while it is empty)
    int64_t s = P, e = F.frame == QE_FRAME_ROWS ? i : F.frame == QE_FRAME_RANGE ? Ge : Pe;
    bool empty = false;
    if (F.frame == QE_FRAME_ROWS_BETWEEN) {  // the bounds are compared, never added before that
      empty = F.lo > F.hi || F.lo > Pe - i || F.hi < P - i;
      s = empty || F.lo <= P - i ? P : i + F.lo;
      e = empty ? P : F.hi >= Pe - i ? Pe : i + F.hi;
    }
    int64_t val = 0;
    bool valid = true;
    switch (F.fn) {
      case QE_WIN_ROW_NUMBER: val = i - P + 1; break;
      case QE_WIN_RANK: val = G - P + 1; break;
      case QE_WIN_DENSE_RANK: val = dense; break;
      case QE_WIN_COUNT_STAR: val = empty ? 0 : e - s + 1; break;
      case QE_WIN_COUNT: val = empty ? 0 : (int64_t)F.scan_f[e] - (s ? (int64_t)F.scan_f[s - 1] : 0); break;
      case QE_WIN_SUM: {
        const int64_t cnt = empty ? 0 : (int64_t)F.scan_f[e] - (s ? (int64_t)F.scan_f[s - 1] : 0);
        valid = cnt > 0;
        if (valid) val = (int64_t)((uint64_t)F.scan_v[e] - (s ? (uint64_t)F.scan_v[s - 1] : 0ull));
        break;
      }
      case QE_WIN_MIN:
      case QE_WIN_MAX: {
        // The forward scan at e covers [max(P, e's block start), e], the backward scan at s covers
        // [s, min(Pe, s's block end)], and a frame is at most one block long: it straddles one block
        // edge (both halves), or starts where the forward scan's segment starts, or ends where the
        // backward scan's segment ends (a frame strictly inside a block is clipped at Pe, or it would
        // be the whole block). Without a block length the only edges are the partition's.
        valid = false;
        if (empty) break;
        const int64_t bs = F.block ? e - (int64_t)((uint32_t)e % (uint32_t)F.block) : 0;
        WinElem r;
        if (s < bs) {
          WinElem l, h;
          l.v = F.back_v[s], l.f = F.back_f[s], l.pad = 0;
          h.v = F.scan_v[e], h.f = F.scan_f[e], h.pad = 0;
          r = win_merge(F.fn == QE_WIN_MAX, F.in_type, l, h);
        } else if (F.scan_f && (s == P || s == bs)) {
          r.v = F.scan_v[e], r.f = F.scan_f[e];
        } else {
          r.v = F.back_v[s], r.f = F.back_f[s];
        }
        valid = (r.f & WF_HAS) != 0;
        if (valid) val = (r.f & WF_SEEDNAN) ? WIN_CANON_NAN : r.v;
        break;
      }
      case QE_WIN_FIRST_VALUE:
      case QE_WIN_LAST_VALUE: {
        valid = false;
        if (empty) break;
        const int64_t rr = C.order[F.fn == QE_WIN_FIRST_VALUE ? s : e];
        if ((uint64_t)rr < (uint64_t)n && row_valid(F.in_valid, rr)) {
          valid = true;
          val = win_value(F.in_type, F.in, rr);
        }
        break;
      }
      default: {  // LAG / LEAD: the offset is compared as an int64, never added before that
        const bool inside = F.fn == QE_WIN_LAG ? F.offset <= i - P : F.offset <= Pe - i;
        valid = false;
        if (inside) {
          const int64_t rr = C.order[F.fn == QE_WIN_LAG ? i - F.offset : i + F.offset];
          if ((uint64_t)rr < (uint64_t)n && row_valid(F.in_valid, rr)) {
            valid = true;
            val = win_value(F.in_type, F.in, rr);
          }
        }
      }
    }
    rec[k] = val;
    valid_bits |= (uint64_t)valid << k;
  }
  rec[A.nfns] = (int64_t)valid_bits;
}

// The staging records cross LDS in both directions, so that global memory sees them as runs of
// consecutive words, never as one 8-byte access per lane at a record's stride (that form of the two
// passes measured 11.8 + 15.8 ms for eight functions over 100M rows). A workgroup of WIN_THREADS takes
// WIN_THREADS positions or rows at a time; in LDS a record has an odd stride (bank spread).
constexpr int WIN_REC_STRIDE = (QE_MAX_AGGS + 1) | 1;
struct WinLds {
  int64_t rec[WIN_THREADS * WIN_REC_STRIDE];
  int32_t pos[WIN_THREADS];
};

// Positions [p0, p0 + WIN_THREADS): one lane per position evaluates into LDS, then the workgroup
// stores the records, which are consecutive in the staging buffer, word by word.
__device__ __forceinline__ void win_eval_block(const WinArgs& A, int64_t p0, WinLds& L) {
  const int W = A.nfns + 1;
  const int64_t i = p0 + threadIdx.x;
  if (i < A.c.n) win_eval_pos(A, i, L.rec + threadIdx.x * WIN_REC_STRIDE);
  __syncthreads();
  const int64_t left = A.c.n - p0;
  const int words = (int)(left < WIN_THREADS ? left : WIN_THREADS) * W;
  for (int x = threadIdx.x; x < words; x += WIN_THREADS) {
    const int row = x / W;
    A.stage[p0 * W + x] = L.rec[row * WIN_REC_STRIDE + (x - row * W)];
  }
  __syncthreads();  // L is rewritten by the next block of positions
}

// Rows [r0, r0 + WIN_THREADS), r0 a multiple of 64: the workgroup gathers the records of positions
// inv[r] into LDS (consecutive lanes read consecutive words of one record), then one lane per input
// row writes the outputs, values coalesced and validity by __ballot. A row no position names (only
// under a bad `order`) gets nulls and zeros.
__device__ __forceinline__ void win_emit_block(const WinArgs& A, int64_t r0, WinLds& L) {
  const int W = A.nfns + 1;
  const int64_t n = A.c.n, nwords = (n + 31) >> 5;
  const int64_t r = r0 + threadIdx.x;
  const bool live = r < n;
  L.pos[threadIdx.x] = live ? A.c.inv[r] : -1;
  __syncthreads();
  for (int x = threadIdx.x; x < WIN_THREADS * W; x += WIN_THREADS) {
    const int row = x / W, k = x - row * W;
    const int64_t i = L.pos[row];
    L.rec[row * WIN_REC_STRIDE + k] = i >= 0 ? A.stage[i * W + k] : 0;
  }
  __syncthreads();
  const int64_t* rec = L.rec + threadIdx.x * WIN_REC_STRIDE;
  const uint64_t valid_bits = (uint64_t)rec[A.nfns];
  const int lane = threadIdx.x & 63;
  const int64_t c = (r0 >> 6) + (threadIdx.x >> 6);
  for (int k = 0; k < A.nfns; ++k) {
    const WinEvalFn& F = A.fns[k];
    const int64_t val = rec[k];
    if (live) {
      if (F.out_width == 8) ((int64_t*)F.out)[r] = val;
      else if (F.out_width == 4) ((int32_t*)F.out)[r] = (int32_t)val;
      else ((uint8_t*)F.out)[r] = (uint8_t)val;
    }
    if (F.out_valid) store_bits64(F.out_valid, c, nwords, __ballot((valid_bits >> k) & 1), lane);
  }
  __syncthreads();  // L is rewritten by the next block of rows
}

// ---- kernels ----------------------------------------------------------------------------------------
// inv[order[i]] = i (inv preset to -1); an entry outside [0, n) writes nothing and sets the flag.
__global__ void __launch_bounds__(256) k_win_inverse(WinCommon C) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < C.n; i += stride) {
    const int64_t r = C.order[i];
    if ((uint64_t)r < (uint64_t)C.n) C.inv[r] = (int32_t)i;
    else *C.flag = 1u;
  }
}

// grid (tiles, jobs): a tile's aggregate.
__global__ void __launch_bounds__(WIN_THREADS) k_win_reduce(WinArgs A) {
  __shared__ WinElem ws[WIN_WAVES];
  const WinJob& J = A.jobs[blockIdx.y];
  const int64_t tile = blockIdx.x;
  if (tile * WIN_TILE >= J.count) return;  // (a word scan has fewer tiles than a position scan)
  const WinElem all = win_scan_tile(J, A.c, tile, win_identity(J.src), WP_REDUCE, ws);
  if (threadIdx.x == 0) A.tile_agg[blockIdx.y * A.tile_stride + tile] = all;
}

// One workgroup per job: tile_carry[t] = the aggregates of tiles 0 .. t-1 combined, in turn.
__global__ void __launch_bounds__(WIN_THREADS) k_win_carry(WinArgs A) {
  __shared__ WinElem ws[WIN_WAVES];
  const WinJob& J = A.jobs[blockIdx.x];
  const int64_t tiles = (J.count + WIN_TILE - 1) / WIN_TILE;
  const WinElem* agg = A.tile_agg + blockIdx.x * A.tile_stride;
  WinElem* carry = A.tile_carry + blockIdx.x * A.tile_stride;
  WinElem run = win_identity(J.src);
  if (threadIdx.x == 0) carry[0] = run;
  for (int64_t t0 = 0; t0 < tiles; t0 += WIN_TILE) {
    WinElem x[WIN_ITEMS];
    const int64_t k0 = t0 + (int64_t)threadIdx.x * WIN_ITEMS;
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) x[j] = k0 + j < tiles ? agg[k0 + j] : win_identity(J.src);
    const WinElem all = win_block_scan(J, x, run, ws);
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j)
      if (k0 + j + 1 < tiles) carry[k0 + j + 1] = x[j];
    run = win_combine(J, run, all);
  }
}

// grid (tiles, jobs): the tile's scan after its carry, stored.
__global__ void __launch_bounds__(WIN_THREADS) k_win_apply(WinArgs A) {
  __shared__ WinElem ws[WIN_WAVES];
  const WinJob& J = A.jobs[blockIdx.y];
  const int64_t tile = blockIdx.x;
  if (tile * WIN_TILE >= J.count) return;
  win_scan_tile(J, A.c, tile, A.tile_carry[blockIdx.y * A.tile_stride + tile], WP_APPLY, ws);
}

// (both: the same trip count in every thread of a workgroup, which meets at barriers inside)
__global__ void __launch_bounds__(WIN_THREADS) k_win_eval(WinArgs A) {
  __shared__ WinLds L;
  for (int64_t p0 = (int64_t)blockIdx.x * WIN_THREADS; p0 < A.c.n; p0 += (int64_t)gridDim.x * WIN_THREADS) win_eval_block(A, p0, L);
}

__global__ void __launch_bounds__(WIN_THREADS) k_win_emit(WinArgs A) {
  __shared__ WinLds L;
  for (int64_t r0 = (int64_t)blockIdx.x * WIN_THREADS; r0 < A.c.n; r0 += (int64_t)gridDim.x * WIN_THREADS) win_emit_block(A, r0, L);
}

// n <= WIN_SMALL_MAX: the whole evaluation in one workgroup. Each __syncthreads also orders the
// workgroup's own global writes before the reads that follow it.
__global__ void __launch_bounds__(WIN_THREADS) k_win_small(WinArgs A) {
  __shared__ WinElem ws[WIN_WAVES];
  __shared__ WinLds L;
  const WinCommon& C = A.c;
  if (threadIdx.x == 0) *C.flag = 0u;
  for (int64_t r = threadIdx.x; r < C.n; r += WIN_THREADS) C.inv[r] = -1;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < C.n; i += WIN_THREADS) {
    const int64_t r = C.order[i];
    if ((uint64_t)r < (uint64_t)C.n) C.inv[r] = (int32_t)i;
    else *C.flag = 1u;
  }
  for (int j = 0; j < A.njobs; ++j) {
    const WinJob& J = A.jobs[j];
    const int64_t tiles = (J.count + WIN_TILE - 1) / WIN_TILE;
    WinElem run = win_identity(J.src);
    for (int64_t t = 0; t < tiles; ++t) run = win_combine(J, run, win_scan_tile(J, C, t, run, WP_ONE, ws));
  }
  __syncthreads();
  for (int64_t p0 = 0; p0 < C.n; p0 += WIN_THREADS) win_eval_block(A, p0, L);
  for (int64_t r0 = 0; r0 < C.n; r0 += WIN_THREADS) win_emit_block(A, r0, L);
}

// ---- boundaries -------------------------------------------------------------------------------------
struct WinKey {
  const void* values;
  const uint8_t* valid;
  const int32_t* offs;
  int32_t type, pad;
};
struct WinKeys {
  WinKey k[QE_MAX_KEYS];
  int32_t n, pad;
};

// Rows a and b differ on some key, by the sort's equality: a null equals a null, every NaN is one
// value, -0.0 != +0.0, UTF8 by bytes.
__device__ __forceinline__ bool win_rows_differ(const WinKeys& K, int64_t a, int64_t b) {
  for (int q = 0; q < K.n; ++q) {
    const WinKey& k = K.k[q];
    const bool va = row_valid(k.valid, a), vb = row_valid(k.valid, b);
    if (va != vb) return true;
    if (!va) continue;
    switch (k.type) {
      case QE_TYPE_INT64:
        if (((const int64_t*)k.values)[a] != ((const int64_t*)k.values)[b]) return true;
        break;
      case QE_TYPE_FLOAT64: {
        int64_t x = ((const int64_t*)k.values)[a], y = ((const int64_t*)k.values)[b];
        if (win_is_nan(x)) x = WIN_CANON_NAN;
        if (win_is_nan(y)) y = WIN_CANON_NAN;
        if (x != y) return true;
        break;
      }
      case QE_TYPE_INT32:
      case QE_TYPE_DATE32:
        if (((const int32_t*)k.values)[a] != ((const int32_t*)k.values)[b]) return true;
        break;
      case QE_TYPE_UINT8:
        if (((const uint8_t*)k.values)[a] != ((const uint8_t*)k.values)[b]) return true;
        break;
      case QE_TYPE_BOOL: {
        const uint8_t* v = (const uint8_t*)k.values;
        if (((v[a >> 3] >> (a & 7)) & 1) != ((v[b >> 3] >> (b & 7)) & 1)) return true;
        break;
      }
      default: {  // UTF8
        const int32_t sa = k.offs[a], sb = k.offs[b];
        const int32_t la = k.offs[a + 1] - sa, lb = k.offs[b + 1] - sb;
        if (la != lb) return true;
        const uint8_t* v = (const uint8_t*)k.values;
        for (int32_t j = 0; j < la; ++j)
          if (v[sa + j] != v[sb + j]) return true;
      }
    }
  }
  return false;
}

__global__ void __launch_bounds__(256) k_win_boundaries(const int32_t* __restrict__ order, int64_t n, WinKeys K,
                                                        uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6, nwords = (n + 31) >> 5;
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t c = wave; c < nchunks; c += nwaves) {  // the same trip count in every lane of a wave
    const int64_t i = c * 64 + lane;
    bool start = false;
    if (i < n) {
      if (i == 0) {
        start = true;
      } else {
        const int64_t a = order[i - 1], b = order[i];
        start = (uint64_t)a >= (uint64_t)n || (uint64_t)b >= (uint64_t)n || win_rows_differ(K, a, b);
      }
    }
    store_bits64(out, c, nwords, __ballot(start), lane);
  }
}

int check_order(const char* who, const qe_column* order, int64_t n) {
  QE_CHECK(order != nullptr, QE_ERR_INVALID_ARG, "%s: null order column", who);
  QE_CHECK(order->type == QE_TYPE_INT32 && !order->validity, QE_ERR_INVALID_ARG,
           "%s: the order column must be INT32 without validity", who);
  QE_CHECK(order->length == n, QE_ERR_INVALID_ARG, "%s: the order column has %lld rows, the input %lld", who,
           (long long)order->length, (long long)n);
  QE_CHECK(order->values || n == 0, QE_ERR_INVALID_ARG, "%s: the order column has no values", who);
  return QE_OK;
}

int check_starts(const char* what, const qe_column* s, int64_t n) {
  QE_CHECK(s != nullptr, QE_ERR_INVALID_ARG, "window_eval: null %s column", what);
  QE_CHECK(s->type == QE_TYPE_BOOL && !s->validity, QE_ERR_INVALID_ARG, "window_eval: %s must be BOOL without validity", what);
  QE_CHECK(s->length == n, QE_ERR_INVALID_ARG, "window_eval: %s has %lld rows, expected %lld", what, (long long)s->length,
           (long long)n);
  QE_CHECK((s->values && ((uintptr_t)s->values & 3) == 0) || n == 0, QE_ERR_INVALID_ARG,
           "window_eval: %s needs a 4-byte aligned values buffer", what);
  return QE_OK;
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int qe_window_layout(int32_t* tile_rows, int32_t* small_max) {
  if (tile_rows) *tile_rows = WIN_TILE;
  if (small_max) *small_max = WIN_SMALL_MAX;
  return QE_OK;
}

int qe_window_boundaries(qe_ctx* ctx, const qe_column* keys, int32_t nkeys, const qe_column* order, qe_column* starts) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(nkeys >= 0 && nkeys <= QE_MAX_KEYS, QE_ERR_INVALID_ARG, "window_boundaries: 0..%d keys, got %d", QE_MAX_KEYS, nkeys);
  QE_CHECK((keys || nkeys == 0) && order && starts, QE_ERR_INVALID_ARG, "window_boundaries: null keys, order or output");
  const int64_t n = order->length;
  QE_CHECK(n >= 0 && n < ((int64_t)1 << 31), QE_ERR_INVALID_ARG, "window_boundaries: %lld rows (at most 2^31 - 1)", (long long)n);
  QE_TRY(check_order("window_boundaries", order, n));
  WinKeys K{};
  K.n = nkeys;
  for (int q = 0; q < nkeys; ++q) {
    const qe_column& c = keys[q];
    QE_CHECK(c.length == n, QE_ERR_INVALID_ARG, "window_boundaries: key %d has %lld rows, the order column %lld", q,
             (long long)c.length, (long long)n);
    QE_CHECK(is_fixed(c.type) || c.type == QE_TYPE_BOOL || c.type == QE_TYPE_UTF8, QE_ERR_UNSUPPORTED,
             "window_boundaries: key %d type %d", q, c.type);
    QE_CHECK(c.values || n == 0, QE_ERR_INVALID_ARG, "window_boundaries: key %d has no values", q);
    QE_CHECK(c.type != QE_TYPE_UTF8 || c.offsets || n == 0, QE_ERR_INVALID_ARG, "window_boundaries: UTF8 key %d needs offsets", q);
    K.k[q] = WinKey{c.values, c.validity, c.offsets, c.type, 0};
  }
  QE_CHECK(starts->type == QE_TYPE_BOOL && !starts->validity, QE_ERR_INVALID_ARG,
           "window_boundaries: the output must be BOOL without validity");
  QE_CHECK(starts->length >= n, QE_ERR_CAPACITY, "window_boundaries: the output holds %lld rows, need %lld",
           (long long)starts->length, (long long)n);
  QE_CHECK((starts->values && ((uintptr_t)starts->values & 3) == 0) || n == 0, QE_ERR_INVALID_ARG,
           "window_boundaries: the output needs a 4-byte aligned values buffer");
  starts->length = n;
  if (n == 0) return QE_OK;
  hipLaunchKernelGGL(k_win_boundaries, dim3(stride_grid(ctx, n)), dim3(256), 0, ctx->stream, (const int32_t*)order->values, n, K,
                     (uint32_t*)starts->values);
  return launch_check("k_win_boundaries");
}

}  // extern "C"

// qe_window_eval (frames_call false: window_check's ids, bounds null) and qe_window_eval_frames.
static int window_eval_impl(qe_ctx* ctx, const qe_column* order, const qe_column* part_starts, const qe_column* peer_starts,
                            const qe_column* inputs, int32_t ninputs, const qe_window_fn* fns, const qe_window_bounds* bounds,
                            int32_t nfns, qe_column* outs, bool frames_call) {
  QE_TRY(ctx_enter(ctx));
  QE_CHECK(part_starts != nullptr, QE_ERR_INVALID_ARG, "window_eval: null partition starts column");
  const int64_t n = part_starts->length;
  QE_CHECK(n >= 0 && n < ((int64_t)1 << 31), QE_ERR_INVALID_ARG, "window_eval: %lld rows (at most 2^31 - 1)", (long long)n);
  QE_TRY(check_order("window_eval", order, n));
  QE_TRY(check_starts("partition starts", part_starts, n));
  QE_TRY(check_starts("peer starts", peer_starts, n));
  QE_CHECK(ninputs >= 0 && ninputs <= QE_MAX_COLS, QE_ERR_INVALID_ARG, "window_eval: 0..%d inputs, got %d", QE_MAX_COLS, ninputs);
  QE_CHECK(nfns >= 0 && nfns <= QE_MAX_AGGS, QE_ERR_INVALID_ARG, "window_eval: 0..%d functions, got %d", QE_MAX_AGGS, nfns);
  QE_CHECK((inputs || ninputs == 0) && ((fns && outs) || nfns == 0), QE_ERR_INVALID_ARG, "window_eval: null column or function arrays");
  for (int c = 0; c < ninputs; ++c)
    QE_CHECK(inputs[c].length == n, QE_ERR_INVALID_ARG, "window_eval: input %d has %lld rows, expected %lld", c,
             (long long)inputs[c].length, (long long)n);
  WinArgs A{};
  for (int k = 0; k < nfns; ++k) {
    const qe_window_fn& f = fns[k];
    QE_CHECK(frames_call ? window_frames_fn_known(f.fn) : window_fn_known(f.fn), QE_ERR_INVALID_ARG,
             "window_eval: function %d: unknown function %d", k, f.fn);
    const bool has_in = window_frames_takes_input(f.fn);
    QE_CHECK(!has_in || (f.input >= 0 && f.input < ninputs), QE_ERR_INVALID_ARG, "window_eval: function %d: input %d outside [0, %d)",
             k, f.input, ninputs);
    const qe_column* in = has_in ? &inputs[f.input] : nullptr;
    int32_t out_type;
    const int st = frames_call ? window_frames_check(f.fn, f.frame, in ? in->type : 0, f.offset, bounds != nullptr, &out_type)
                               : window_check(f.fn, f.frame, in ? in->type : 0, f.offset, &out_type);
    QE_CHECK(st == QE_OK, st, "window_eval: function %d (fn %d, frame %d, input type %d, offset %lld) is %s", k, f.fn, f.frame,
             in ? in->type : 0, (long long)f.offset, st == QE_ERR_UNSUPPORTED ? "not supported" : "not valid");
    const bool reads = has_in && f.fn != QE_WIN_COUNT;
    QE_CHECK(!reads || in->values || n == 0, QE_ERR_INVALID_ARG, "window_eval: input %d has no values", f.input);
    const qe_column& o = outs[k];
    QE_CHECK(o.type == out_type, QE_ERR_INVALID_ARG, "window_eval: output %d must have type %d, has %d", k, out_type, o.type);
    QE_CHECK(o.length >= n, QE_ERR_CAPACITY, "window_eval: output %d holds %lld rows, need %lld", k, (long long)o.length, (long long)n);
    QE_CHECK(o.values || n == 0, QE_ERR_INVALID_ARG, "window_eval: output %d has no values", k);
    QE_CHECK((o.validity || !window_frames_nullable(f.fn)) && ((uintptr_t)o.validity & 3) == 0, QE_ERR_INVALID_ARG,
             "window_eval: output %d needs a 4-byte aligned validity buffer (its result can be null)", k);
    WinEvalFn& F = A.fns[k];
    F.fn = f.fn;
    F.frame = f.frame;
    F.in_type = in ? in->type : 0;
    F.out_width = type_width(out_type);
    F.offset = f.offset;
    if (f.frame == QE_FRAME_ROWS_BETWEEN) {
      F.lo = window_clamp_bound(bounds[k].lo, n);
      F.hi = window_clamp_bound(bounds[k].hi, n);
    }
    F.in = in ? in->values : nullptr;
    F.in_valid = in ? in->validity : nullptr;
    F.out = o.values;
    F.out_valid = (uint32_t*)o.validity;
    A.need_dense |= f.fn == QE_WIN_DENSE_RANK;
  }
  for (int k = 0; k < nfns; ++k) outs[k].length = n;
  if (n == 0 || nfns == 0) return QE_OK;

  const WindowFrameScans S = window_frame_scans(fns, bounds, nfns, n);
  const int64_t nw = window_words(n), tiles = window_tiles(n);
  Blocks blk(ctx);
  char* p;
  QE_TRY(blk.alloc((size_t)window_frames_work_bytes(n, fns, bounds, nfns), (void**)&p));
  A.c = WinCommon{(const int32_t*)order->values, (const uint32_t*)part_starts->values, (const uint32_t*)peer_starts->values, n, nw,
                  nullptr, (unsigned*)p};
  p += WIN_HEAD_BYTES;
  A.c.inv = (int32_t*)p;
  p += window_inv_bytes(n);
  int32_t* words[WIN_WORD_SCANS];
  for (int j = 0; j < WIN_WORD_SCANS; ++j, p += window_word_bytes(n)) words[j] = (int32_t*)p;
  A.prev_part = words[0];
  A.next_part = words[1];
  A.prev_peer = words[2];
  A.next_peer = words[3];
  A.cum_peer = words[4];
  const int32_t word_src[WIN_WORD_SCANS] = {WS_PREV, WS_NEXT, WS_PREV, WS_NEXT, WS_POPC};
  for (int j = 0; j < WIN_WORD_SCANS; ++j)
    A.jobs[j] = WinJob{word_src[j], 0, 0, 0, j < 2 ? A.c.part : A.c.peer, nullptr, nullptr, nw, nullptr, words[j]};
  A.njobs = WIN_WORD_SCANS + S.n;
  A.nfns = nfns;
  for (int j = 0; j < S.n; ++j) {
    const qe_column& in = inputs[S.input[j]];
    int64_t* v = (int64_t*)p;
    p += window_scan_value_bytes(n);
    int32_t* f = (int32_t*)p;
    p += window_scan_flag_bytes(n);
    const int32_t src = S.kind[j] == WIN_SCAN_SUM ? WS_SUM : S.kind[j] == WIN_SCAN_MIN ? WS_MIN : WS_MAX;
    A.jobs[WIN_WORD_SCANS + j] = WinJob{src, in.type, S.back[j], (uint32_t)S.block[j], nullptr, in.values, in.validity, n, v, f};
  }
  for (int k = 0; k < nfns; ++k) {
    if (S.fwd_of_fn[k] >= 0) {
      A.fns[k].scan_v = A.jobs[WIN_WORD_SCANS + S.fwd_of_fn[k]].out_v;
      A.fns[k].scan_f = A.jobs[WIN_WORD_SCANS + S.fwd_of_fn[k]].out_f;
      A.fns[k].block = S.block[S.fwd_of_fn[k]];
    }
    if (S.bwd_of_fn[k] >= 0) {
      A.fns[k].back_v = A.jobs[WIN_WORD_SCANS + S.bwd_of_fn[k]].out_v;
      A.fns[k].back_f = A.jobs[WIN_WORD_SCANS + S.bwd_of_fn[k]].out_f;
      A.fns[k].block = S.block[S.bwd_of_fn[k]];
    }
  }
  A.tile_agg = (WinElem*)p;
  p += window_tile_bytes(n, S.n);
  A.tile_carry = (WinElem*)p;
  p += window_tile_bytes(n, S.n);
  A.stage = (int64_t*)p;
  A.tile_stride = tiles + 1;

  if (n <= WIN_SMALL_MAX) {
    hipLaunchKernelGGL(k_win_small, dim3(1), dim3(WIN_THREADS), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_small"));
  } else {
    QE_HIP(hipMemsetAsync(A.c.flag, 0, 4, ctx->stream));
    QE_HIP(hipMemsetAsync(A.c.inv, 0xFF, (size_t)n * 4, ctx->stream));
    const int grid = stride_grid(ctx, n);
    hipLaunchKernelGGL(k_win_inverse, dim3(grid), dim3(256), 0, ctx->stream, A.c);
    QE_TRY(launch_check("k_win_inverse"));
    hipLaunchKernelGGL(k_win_reduce, dim3((unsigned)tiles, (unsigned)A.njobs), dim3(WIN_THREADS), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_reduce"));
    hipLaunchKernelGGL(k_win_carry, dim3((unsigned)A.njobs), dim3(WIN_THREADS), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_carry"));
    hipLaunchKernelGGL(k_win_apply, dim3((unsigned)tiles, (unsigned)A.njobs), dim3(WIN_THREADS), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_apply"));
    hipLaunchKernelGGL(k_win_eval, dim3(grid), dim3(256), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_eval"));
    hipLaunchKernelGGL(k_win_emit, dim3(grid), dim3(256), 0, ctx->stream, A);
    QE_TRY(launch_check("k_win_emit"));
  }
  // the out-of-range flag: the call's one read-back (as qe_take reads its own)
  void* hp;
  QE_TRY(ctx_pinned(ctx, 8, &hp));
  QE_HIP(hipMemcpyAsync(hp, A.c.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  QE_TRY(ctx_sync(ctx));
  QE_CHECK(*(const unsigned*)hp == 0, QE_ERR_INVALID_ARG, "window_eval: an order entry is outside [0, %lld)", (long long)n);
  return QE_OK;
}

extern "C" {

int qe_window_eval(qe_ctx* ctx, const qe_column* order, const qe_column* part_starts, const qe_column* peer_starts,
                   const qe_column* inputs, int32_t ninputs, const qe_window_fn* fns, int32_t nfns, qe_column* outs) {
  return window_eval_impl(ctx, order, part_starts, peer_starts, inputs, ninputs, fns, nullptr, nfns, outs, false);
}

int qe_window_eval_frames(qe_ctx* ctx, const qe_column* order, const qe_column* part_starts, const qe_column* peer_starts,
                          const qe_column* inputs, int32_t ninputs, const qe_window_fn* fns, const qe_window_bounds* bounds,
                          int32_t nfns, qe_column* outs) {
  return window_eval_impl(ctx, order, part_starts, peer_starts, inputs, ninputs, fns, bounds, nfns, outs, true);
}

}  // extern "C"
