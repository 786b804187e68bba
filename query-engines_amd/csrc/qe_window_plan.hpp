// qe_window_plan.hpp — the host-side rules of the window functions as plain
// functions of numbers: which function x type x frame combinations qe_window_eval accepts and with
// which status it refuses the others, the output types, which scan over the sorted positions each
// function reads, and the working memory of a call. Plain C++17: qe_window.hip uses them and keeps no
// second copy, and tests/native/window_plan_host.cpp (g++) holds them to tests/windowref.py without a
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

}  // namespace qe
