// qe_window_plan.hpp — the host-side rules of the window functions as plain
// functions of numbers: which function x type x frame combinations qe_window_eval accepts and with
// which status it refuses the others, the output types, which scan over the sorted positions each
// function reads, and the working memory of a call; then the same for qe_window_eval_frames (two more
// functions, the frame ROWS BETWEEN lo AND hi, forward and backward block scans). Plain C++17:
// qe_window.hip uses them and keeps no second copy, and tests/native/window_plan_host.cpp and
// window_frames_host.cpp (g++) hold them to tests/windowref.py and tests/windowframeref.py without a
// GPU.
#pragma once

#include <stdint.h>

#include "qe_hip.h"

namespace qe {

// Positions per tile of the multi-workgroup scans (WIN_THREADS threads x WIN_ITEMS consecutive
// positions each), and the largest n the one-workgroup kernel takes (it walks its tiles in turn).
constexpr int WIN_THREADS = 256;
constexpr int WIN_ITEMS = 8;
constexpr int WIN_TILE = WIN_THREADS * WIN_ITEMS;
constexpr int WIN_SMALL_MAX = 2 * WIN_TILE;
// Scans over the words of the two boundary bitmaps that every call runs: the last set bit at or
// before each word and the first at or after it, for both bitmaps, and the peer bitmap's running
// popcount.
constexpr int WIN_WORD_SCANS = 5;

// The scan over sorted positions that a function reads.
enum { WIN_SCAN_NONE = 0, WIN_SCAN_SUM = 1, WIN_SCAN_MIN = 2, WIN_SCAN_MAX = 3 };

inline bool window_fn_known(int32_t fn) { return fn >= QE_WIN_ROW_NUMBER && fn <= QE_WIN_LEAD; }
inline bool window_frame_known(int32_t frame) { return frame >= QE_FRAME_ROWS && frame <= QE_FRAME_PARTITION; }
inline bool window_takes_input(int32_t fn) { return fn >= QE_WIN_COUNT && fn <= QE_WIN_LEAD; }
inline bool window_takes_offset(int32_t fn) { return fn == QE_WIN_LAG || fn == QE_WIN_LEAD; }
// The result can be null: its output needs a validity buffer.
inline bool window_nullable(int32_t fn) { return fn >= QE_WIN_SUM && fn <= QE_WIN_LEAD; }

// SUM and COUNT(x) share one scan: the running (wrapping sum, non-null count) pair.
inline int32_t window_scan_of(int32_t fn) {
  switch (fn) {
    case QE_WIN_COUNT:
    case QE_WIN_SUM: return WIN_SCAN_SUM;
    case QE_WIN_MIN: return WIN_SCAN_MIN;
    case QE_WIN_MAX: return WIN_SCAN_MAX;
    default: return WIN_SCAN_NONE;
  }
}

inline bool window_type_known(int32_t t) { return t >= QE_TYPE_INT64 && t <= QE_TYPE_DATE32; }
inline bool window_type_value(int32_t t) {  // a type MIN / MAX / LAG / LEAD carry
  return t == QE_TYPE_INT64 || t == QE_TYPE_FLOAT64 || t == QE_TYPE_INT32 || t == QE_TYPE_DATE32 || t == QE_TYPE_UINT8;
}

// One function of a call: QE_OK and the output type, or the status it is refused with. in_type: the
// type of the column fns[k].input names (ignored by the functions without an input).
inline int window_check(int32_t fn, int32_t frame, int32_t in_type, int64_t offset, int32_t* out_type) {
  *out_type = 0;
  if (!window_fn_known(fn) || !window_frame_known(frame)) return QE_ERR_INVALID_ARG;
  if (window_takes_offset(fn) && offset < 0) return QE_ERR_INVALID_ARG;
  if (!window_takes_input(fn) || fn == QE_WIN_COUNT) {
    if (fn == QE_WIN_COUNT && !window_type_known(in_type)) return QE_ERR_INVALID_ARG;
    *out_type = QE_TYPE_INT64;
    return QE_OK;
  }
  if (!window_type_known(in_type)) return QE_ERR_INVALID_ARG;
  if (fn == QE_WIN_SUM) {
    // FLOAT64: §4 promises the correctly rounded exact sum, and an exact prefix sum is not built
    if (in_type != QE_TYPE_INT64 && in_type != QE_TYPE_INT32) return QE_ERR_UNSUPPORTED;
    *out_type = QE_TYPE_INT64;
    return QE_OK;
  }
  if (!window_type_value(in_type)) return QE_ERR_UNSUPPORTED;  // BOOL, UTF8
  *out_type = in_type;
  return QE_OK;
}

// The distinct (scan, input) pairs of a call's functions, in order of first use.
struct WindowScans {
  int32_t n = 0;
  int32_t kind[QE_MAX_AGGS] = {};
  int32_t input[QE_MAX_AGGS] = {};
  int32_t of_fn[QE_MAX_AGGS] = {};  // index of function k's scan, -1 when it reads none
};

inline WindowScans window_scans(const qe_window_fn* fns, int32_t nfns) {
  WindowScans S;
  for (int32_t k = 0; k < nfns && k < QE_MAX_AGGS; ++k) {
    const int32_t kind = window_scan_of(fns[k].fn);
    S.of_fn[k] = -1;
    if (kind == WIN_SCAN_NONE) continue;
    for (int32_t j = 0; j < S.n; ++j)
      if (S.kind[j] == kind && S.input[j] == fns[k].input) S.of_fn[k] = j;
    if (S.of_fn[k] < 0) {
      S.kind[S.n] = kind;
      S.input[S.n] = fns[k].input;
      S.of_fn[k] = S.n++;
    }
  }
  return S;
}

inline int64_t window_align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline int64_t window_words(int64_t n) { return (n + 31) / 32; }
inline int64_t window_tiles(int64_t n) { return (n + WIN_TILE - 1) / WIN_TILE; }

// Sections of a call's working memory, each a multiple of 256 bytes:
// [head: flag | inverse permutation | WIN_WORD_SCANS word arrays | per scan: values, counts / flags |
//  tile aggregates and tile carries of every scan | staging records]
constexpr int64_t WIN_HEAD_BYTES = 256;
constexpr int64_t WIN_ELEM_BYTES = 16;  // one scan element (value, count or flags)
inline int64_t window_inv_bytes(int64_t n) { return window_align256(4 * n); }
inline int64_t window_word_bytes(int64_t n) { return window_align256(4 * window_words(n)); }
inline int64_t window_scan_value_bytes(int64_t n) { return window_align256(8 * n); }
inline int64_t window_scan_flag_bytes(int64_t n) { return window_align256(4 * n); }
inline int64_t window_tile_bytes(int64_t n, int32_t nscans) {
  return window_align256((int64_t)(WIN_WORD_SCANS + nscans) * (window_tiles(n) + 1) * WIN_ELEM_BYTES);
}
// the staging records: per position every function's value, then one word of validity bits
inline int64_t window_stage_bytes(int64_t n, int32_t nfns) { return window_align256(8 * n * (nfns + 1)); }
inline int64_t window_work_bytes(int64_t n, int32_t nscans, int32_t nfns) {
  return WIN_HEAD_BYTES + window_inv_bytes(n) + WIN_WORD_SCANS * window_word_bytes(n) +
         (int64_t)nscans * (window_scan_value_bytes(n) + window_scan_flag_bytes(n)) + 2 * window_tile_bytes(n, nscans) +
         window_stage_bytes(n, nfns);
}

// ---- qe_window_eval_frames: FIRST_VALUE / LAST_VALUE and the QE_FRAME_ROWS_BETWEEN frame ---------------
// The rules above widened by two functions and one frame; qe_window_eval keeps the rules above.
inline bool window_frames_fn_known(int32_t fn) { return fn >= QE_WIN_ROW_NUMBER && fn <= QE_WIN_LAST_VALUE; }
inline bool window_frames_frame_known(int32_t frame) { return frame >= QE_FRAME_ROWS && frame <= QE_FRAME_ROWS_BETWEEN; }
inline bool window_frames_takes_input(int32_t fn) { return fn >= QE_WIN_COUNT && fn <= QE_WIN_LAST_VALUE; }
inline bool window_frames_nullable(int32_t fn) { return fn >= QE_WIN_SUM && fn <= QE_WIN_LAST_VALUE; }

// window_check for the wider ids. has_bounds: the call passed a bounds array (QE_FRAME_ROWS_BETWEEN
// needs one, whatever the function; the bounds' values are never a reason to refuse).
inline int window_frames_check(int32_t fn, int32_t frame, int32_t in_type, int64_t offset, bool has_bounds, int32_t* out_type) {
  *out_type = 0;
  if (!window_frames_fn_known(fn) || !window_frames_frame_known(frame)) return QE_ERR_INVALID_ARG;
  if (frame == QE_FRAME_ROWS_BETWEEN && !has_bounds) return QE_ERR_INVALID_ARG;
  if (fn == QE_WIN_FIRST_VALUE || fn == QE_WIN_LAST_VALUE) {  // the types LAG takes; no offset
    if (!window_type_known(in_type)) return QE_ERR_INVALID_ARG;
    if (!window_type_value(in_type)) return QE_ERR_UNSUPPORTED;
    *out_type = in_type;
    return QE_OK;
  }
  return window_check(fn, frame == QE_FRAME_ROWS_BETWEEN ? QE_FRAME_ROWS : frame, in_type, offset, out_type);
}

// A bound clamped to [-n, n]: no frame changes (a partition has at most n rows, so i + lo < P for every
// lo <= -n and i + lo > Pe for every lo >= n, and likewise for hi), and hi - lo + 1 cannot overflow.
inline int64_t window_clamp_bound(int64_t b, int64_t n) { return b < -n ? -n : b > n ? n : b; }

// The scans over positions of a qe_window_eval_frames call. A scan is (kind, input, direction, block
// length): forward scans restart where a partition starts and, with a block length L > 0, where
// position % L == 0; backward scans run from the right and restart where a partition ends and where
// position % L == L - 1. Block length 0: partitions only. (kind, input, forward, 0) is the scan of
// window_scans, so a call without bounded MIN / MAX has window_scans' list.
//   SUM / COUNT(x), any frame: the running pair, forward, 0 (a frame's value is S[e] - S[s-1]).
//   MIN / MAX under the three older frames: forward, 0.
//   MIN / MAX under QE_FRAME_ROWS_BETWEEN, (lo, hi) clamped to [-n, n]:
//     lo > hi            every frame is empty: no scan
//     lo == -n           s = P for every row: forward, 0, read at e
//     hi == n            e = Pe for every row: backward, 0, read at s
//     otherwise          L = hi - lo + 1 bounds a frame's width: forward and backward with block length L,
//                        or 0 when L >= n (one block would cover every position)
struct WindowFrameScans {
  int32_t n = 0;
  int32_t kind[2 * QE_MAX_AGGS] = {};
  int32_t input[2 * QE_MAX_AGGS] = {};
  int32_t back[2 * QE_MAX_AGGS] = {};
  int64_t block[2 * QE_MAX_AGGS] = {};
  int32_t fwd_of_fn[QE_MAX_AGGS] = {};  // index of the forward scan function k reads, -1 when none
  int32_t bwd_of_fn[QE_MAX_AGGS] = {};  // ... of the backward scan
};

inline int32_t window_frame_scan_slot(WindowFrameScans& S, int32_t kind, int32_t input, int32_t back, int64_t block) {
  for (int32_t j = 0; j < S.n; ++j)
    if (S.kind[j] == kind && S.input[j] == input && S.back[j] == back && S.block[j] == block) return j;
  S.kind[S.n] = kind;
  S.input[S.n] = input;
  S.back[S.n] = back;
  S.block[S.n] = block;
  return S.n++;
}

// bounds may be null when no function has frame QE_FRAME_ROWS_BETWEEN.
inline WindowFrameScans window_frame_scans(const qe_window_fn* fns, const qe_window_bounds* bounds, int32_t nfns, int64_t n) {
  WindowFrameScans S;
  for (int32_t k = 0; k < nfns && k < QE_MAX_AGGS; ++k) {
    const int32_t kind = window_scan_of(fns[k].fn);
    S.fwd_of_fn[k] = S.bwd_of_fn[k] = -1;
    if (kind == WIN_SCAN_NONE) continue;
    if (kind == WIN_SCAN_SUM || fns[k].frame != QE_FRAME_ROWS_BETWEEN || !bounds) {
      S.fwd_of_fn[k] = window_frame_scan_slot(S, kind, fns[k].input, 0, 0);
      continue;
    }
    const int64_t lo = window_clamp_bound(bounds[k].lo, n), hi = window_clamp_bound(bounds[k].hi, n);
    if (lo > hi) continue;
    if (lo == -n) {
      S.fwd_of_fn[k] = window_frame_scan_slot(S, kind, fns[k].input, 0, 0);
    } else if (hi == n) {
      S.bwd_of_fn[k] = window_frame_scan_slot(S, kind, fns[k].input, 1, 0);
    } else {
      const int64_t L = hi - lo + 1, block = L >= n ? 0 : L;
      S.fwd_of_fn[k] = window_frame_scan_slot(S, kind, fns[k].input, 0, block);
      S.bwd_of_fn[k] = window_frame_scan_slot(S, kind, fns[k].input, 1, block);
    }
  }
  return S;
}

// Working memory of a qe_window_eval_frames call: window_work_bytes with this call's scans.
inline int64_t window_frames_work_bytes(int64_t n, const qe_window_fn* fns, const qe_window_bounds* bounds, int32_t nfns) {
  return window_work_bytes(n, window_frame_scans(fns, bounds, nfns, n).n, nfns);
}

}  // namespace qe
