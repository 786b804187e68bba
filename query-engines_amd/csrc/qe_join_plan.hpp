// qe_join_plan.hpp — the equi-join's key word, type pairing, table size and home slot (DESIGN §4 /
// §6.11) as plain functions of numbers. Compiled for the device by qe_join.hip, whose kernels and
// qe_join_build keep no second copy, and for the host by tests/native/join_plan_host.cpp (g++), so
// the NaN, ±0, sign-extension and sentinel rules are tested without a GPU.
//
// Key word: one 64-bit word per non-null row; two rows join iff their words are equal.
//   INT64            the value
//   INT32 / DATE32   sign-extended (INT32 -1 == INT64 -1)
//   UINT8 / BOOL     zero-extended (UINT8 255 != INT32 -1)
//   FLOAT64          the IEEE bits with every NaN replaced by the one quiet pattern: Double.equals, as
//                    the group keys apply it (every NaN one key, -0.0 != +0.0). FLOAT64 pairs only
//                    with FLOAT64: 1.0 and the integer 0x3FF0000000000000 share a word.
// Table: open addressing, linear probing, slots = the least power of two >= max(64, 2 x non-null
// build rows); home slot = fmix64(key word) & (slots - 1). Every 64-bit value is a legal key word:
// the word JOIN_EMPTY_WORD marks a free slot in the key array and, as a key, lives in the side slot
// `slots` (one past the probed range), as EMPTY_KEY does in the GROUP BY tables.
// Match marks (RIGHT / FULL OUTER and the build-side semi / anti joins): one bit per slot, the side
// slot included; the probe kinds that set them are decoded here (tests/native/join_marks_host.cpp).
#pragma once

#include <stdint.h>

#include "qe_hip.h"

#if defined(__HIPCC__)
#include "qe_dev.hpp"  // fmix64
#define QE_JOIN_HD __host__ __device__ __forceinline__
#else
#define QE_JOIN_HD inline
namespace qe {
// qe_dev.hpp needs a HIP compiler; the host build restates its murmur3 finaliser, and
// tests/test_join_host.py holds join_home to the same function written in Python.
inline unsigned long long fmix64(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}
}  // namespace qe
#endif

namespace qe {

constexpr uint64_t JOIN_CANON_NAN = 0x7FF8000000000000ull;
constexpr uint64_t JOIN_EMPTY_WORD = ~0ull;  // (a byte fill clears the table)
constexpr int64_t JOIN_MIN_SLOTS = 64;
constexpr int64_t JOIN_MAX_ROWS = 0x7FFFFFFFll;  // build rows, probe rows per call, pairs per call

QE_JOIN_HD bool join_key_type(int32_t type) {
  switch (type) {
    case QE_TYPE_INT64:
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32:
    case QE_TYPE_UINT8:
    case QE_TYPE_BOOL:
    case QE_TYPE_FLOAT64: return true;
    default: return false;
  }
}

// Whether a build key of type `build` joins with a probe key of type `probe`.
QE_JOIN_HD bool join_compatible(int32_t build, int32_t probe) {
  return join_key_type(build) && join_key_type(probe) && (build == QE_TYPE_FLOAT64) == (probe == QE_TYPE_FLOAT64);
}

// The key word of the raw value `raw` (the column's bits in the low bits; the rest is ignored).
QE_JOIN_HD uint64_t join_key_word(int32_t type, uint64_t raw) {
  switch (type) {
    case QE_TYPE_INT64: return raw;
    case QE_TYPE_FLOAT64: return (raw & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull ? JOIN_CANON_NAN : raw;
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32: return (uint64_t)(int64_t)(int32_t)(uint32_t)raw;
    case QE_TYPE_UINT8: return raw & 0xFFu;
    default: return raw & 1u;  // BOOL
  }
}

// Slots of the table of `rows` non-null build rows.
QE_JOIN_HD int64_t join_slots(int64_t rows) {
  int64_t s = JOIN_MIN_SLOTS;
  while (s < 2 * rows) s <<= 1;
  return s;
}

QE_JOIN_HD uint64_t join_home(uint64_t word, uint64_t slots) { return (uint64_t)fmix64(word) & (slots - 1); }

// qe_join_probe's `kind`: QE_JOIN_INNER or QE_JOIN_LEFT, alone or with the QE_JOIN_TRACK bit (the
// probe then marks the build keys it matches). false: any other value, refused.
QE_JOIN_HD bool join_probe_kind(int32_t kind, int32_t* base, bool* track) {
  *base = kind & ~(int32_t)QE_JOIN_TRACK;
  *track = (kind & QE_JOIN_TRACK) != 0;
  return *base == QE_JOIN_INNER || *base == QE_JOIN_LEFT;
}

// Match marks: one bit per slot of [0, slots], the side slot `slots` included, in 32-bit words.
QE_JOIN_HD int64_t join_mark_words(int64_t slots) { return (slots + 1 + 31) >> 5; }
QE_JOIN_HD uint64_t join_mark_word(uint64_t slot) { return slot >> 5; }
QE_JOIN_HD uint32_t join_mark_bit(uint64_t slot) { return 1u << (slot & 31); }

}  // namespace qe
