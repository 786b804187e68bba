// Order-preserving sort-key encoders (ORDER BY). Plain C++: compiled for the
// device by qe_sort.hip and for the host by tests/native/sort_key_host.cpp (g++), so the NaN, ±0,
// null-placement and DESC rules are tested without a GPU.
//
// A key value becomes `sort_value_bits(type)` unsigned bits in which smaller means earlier; a
// nullable key adds one null bit ABOVE them. The pair (null bit, value bits) compared as one
// unsigned number is the key's order:
//   value bits : signed integers flip the sign bit; fp64 flips the sign bit of non-negative values
//                and every bit of negative ones, after every NaN became the one quiet pattern above
//                +Inf (java.lang.Double.compare: -Inf < ... < -0.0 < +0.0 < ... < +Inf < NaN, all
//                NaNs equal); QE_SORT_DESC stores the bitwise NOT; a null row stores 0.
//   null bit   : QE_SORT_NULLS_FIRST: 0 for null, 1 for a value; otherwise 1 for null, 0 for a
//                value. DESC never touches it.
#pragma once

#include <stdint.h>

#include "qe_hip.h"

#if defined(__HIPCC__)
#define QE_SORT_HD __host__ __device__ __forceinline__
#else
#define QE_SORT_HD inline
#endif

namespace qe {

constexpr uint64_t SORT_SIGN64 = 0x8000000000000000ull;
constexpr uint64_t SORT_CANON_NAN = 0x7FF8000000000000ull;

// Value bits of a fixed-width or BOOL key (0: not such a type).
QE_SORT_HD int sort_value_bits(int32_t type) {
  switch (type) {
    case QE_TYPE_INT64:
    case QE_TYPE_FLOAT64: return 64;
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32: return 32;
    case QE_TYPE_UINT8: return 8;
    case QE_TYPE_BOOL: return 1;
    default: return 0;
  }
}

QE_SORT_HD uint64_t sort_low_mask(int bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1); }

QE_SORT_HD uint64_t sort_enc_i64(int64_t v) { return (uint64_t)v ^ SORT_SIGN64; }
QE_SORT_HD uint64_t sort_enc_i32(int32_t v) { return (uint64_t)((uint32_t)v ^ 0x80000000u); }
QE_SORT_HD uint64_t sort_enc_u8(uint8_t v) { return v; }
QE_SORT_HD uint64_t sort_enc_bool(bool v) { return v ? 1 : 0; }
QE_SORT_HD uint64_t sort_enc_f64(uint64_t bits) {
  if ((bits & ~SORT_SIGN64) > 0x7FF0000000000000ull) bits = SORT_CANON_NAN;  // any NaN, either sign
  return (bits & SORT_SIGN64) ? ~bits : (bits | SORT_SIGN64);
}

// Ascending value bits of the raw value `raw` (the column's bits, zero- or sign-extended: only the
// type's low bits are read).
QE_SORT_HD uint64_t sort_enc_fixed(int32_t type, uint64_t raw) {
  switch (type) {
    case QE_TYPE_INT64: return sort_enc_i64((int64_t)raw);
    case QE_TYPE_FLOAT64: return sort_enc_f64(raw);
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32: return sort_enc_i32((int32_t)(uint32_t)raw);
    case QE_TYPE_UINT8: return sort_enc_u8((uint8_t)raw);
    default: return sort_enc_bool((raw & 1) != 0);
  }
}

// The stored value field of `bits` bits: `asc` as the ascending encoders give it.
QE_SORT_HD uint64_t sort_field(uint64_t asc, int bits, bool valid, int32_t flags) {
  if (!valid) return 0;
  return ((flags & QE_SORT_DESC) ? ~asc : asc) & sort_low_mask(bits);
}

QE_SORT_HD uint64_t sort_null_bit(bool valid, int32_t flags) {
  return (flags & QE_SORT_NULLS_FIRST) ? (valid ? 1 : 0) : (valid ? 0 : 1);
}

// Bits of a field whose least significant bit is bit `lo` of the whole key (bit 0 = the least
// significant bit of the last word) that fall into word k, where word k holds key bits
// [64 k, 64 k + 64).
QE_SORT_HD uint64_t sort_place(uint64_t field, int64_t lo, int64_t k) {
  const int64_t d = lo - 64 * k;
  if (d >= 64 || d <= -64) return 0;
  return d >= 0 ? field << d : field >> (-d);
}

}  // namespace qe
