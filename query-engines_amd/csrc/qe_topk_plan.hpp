// qe_topk_plan.hpp — the host-side rules of the top-k radix selection as plain
// functions of numbers: the threshold-bin pick, the `need` bookkeeping, the stop rule and the
// QE_TOPK_AUTO rule. Plain C++17: qe_sort.hip's qe_topk_indices uses them and keeps no second
// copy, and tests/native/topk_plan_host.cpp (g++) holds them to tests/topkref.py without a GPU.
//
// The selection keeps a candidate list C of rows that holds every row of the true top-k. A row of C
// is SURE (its key prefix is strictly below the threshold prefix found so far: it is in the top-k
// whatever its lower digits are) or TIED (equal to it). One digit step histograms the next 8-bit
// digit of the tied rows, picks the bin in which the k-th row lies, and keeps the rows at or below
// it: the rows below it become sure.
#pragma once

#include <stdint.h>

namespace qe {

// The selection stops, and the candidates are sorted, once |C| <= max(small_max, TOPK_STOP_FACTOR * k).
// A/B at 100M rows (factors 1, 2, 4, 8): docs/experiments.md "Top-k stop factor".
#ifndef QE_TOPK_STOP_FACTOR
#define QE_TOPK_STOP_FACTOR 2
#endif
// QE_TOPK_AUTO selects when k <= n / QE_TOPK_AUTO_DIV. Measured (DESIGN §9 "top-k", full-range INT64,
// ms select / sort): at k = n / 4, the largest k timed, selection is still ahead at 10M rows
// (0.88 / 0.92) and at 100M (6.0 / 9.6), so the crossover lies above n / 4; half of that bound, as
// the margin for other key shapes, is n / 8. (Keys with few varying digits, where the full sort
// runs 3 passes, lose at every k: 4.7 / 3.6 at 100M rows in [0, 2^20). AUTO does not see that.)
#ifndef QE_TOPK_AUTO_DIV
#define QE_TOPK_AUTO_DIV 8
#endif

struct TopkPick {
  int32_t bin;     // the threshold bin b: below(b) < need <= below(b) + hist[b]; -1: need is not in 1..total
  int64_t below;   // rows in the bins under b: they become sure
  int64_t tied;    // hist[b]: they stay tied
};

// The bin of a 256-bin digit histogram that holds the need-th smallest row (need counts from 1).
inline TopkPick topk_pick_bin(const uint32_t* hist, int64_t need) {
  int64_t below = 0;  // (64 bits: one bin may hold 2^31 - 1 rows)
  if (need >= 1) {
    for (int32_t b = 0; b < 256; ++b) {
      if (need <= below + (int64_t)hist[b]) return TopkPick{b, below, (int64_t)hist[b]};
      below += (int64_t)hist[b];
    }
  }
  return TopkPick{-1, below, 0};
}

// The highest of the 8 digits of a word (hist8[256 g + v]: digit g, value v, g = 7 the most
// significant) that is not the same in all `rows` histogrammed rows; -1: the word is constant.
inline int32_t topk_top_digit(const uint32_t* hist8, int64_t rows) {
  for (int32_t g = 7; g >= 0; --g) {
    bool constant = false;
    for (int v = 0; v < 256; ++v) constant |= (int64_t)hist8[256 * g + v] == rows;
    if (!constant) return g;
  }
  return -1;
}

// The candidate list between digit steps: |C| = sure + tied, and `k - sure` of the tied rows are
// still to be found.
struct TopkNeed {
  int64_t k, sure, tied;
  int64_t need() const { return k - sure; }
  int64_t candidates() const { return sure + tied; }
  void take(const TopkPick& p) {
    sure += p.below;
    tied = p.tied;
  }
  // After the last digit of the last word the tied rows are equal on every key: the first need() of
  // them in row order are the rest of the top-k.
  void cut() { tied = need(); }
};

// (candidates <= FACTOR * k, written without the product: k may be any int64.)
inline bool topk_stop(int64_t candidates, int64_t k, int64_t small_max) {
  return candidates <= small_max || (candidates - 1) / (int64_t)QE_TOPK_STOP_FACTOR < k;
}

// QE_TOPK_AUTO: the full sort when it is one launch (n <= small_max) or nothing is cut (k >= n),
// selection when k <= n / QE_TOPK_AUTO_DIV; monotone in k (select below a bound, sort from it on).
inline bool topk_use_select(int64_t n, int64_t k, int64_t small_max) {
  if (n <= small_max || k >= n) return false;
  return k <= n / QE_TOPK_AUTO_DIV;
}

}  // namespace qe
