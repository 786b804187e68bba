// Shared by the operators that work on row indices (qe_sort.hip, qe_take.hip, qe_join.hip,
// qe_window.hip): reading a row of a column, writing a wave's result bits, and a call's working
// memory and grid-stride launch width on the host.
#pragma once

#include "qe_internal.hpp"

#include <vector>

namespace qe {

// Row r is not null. A column without a validity buffer has no nulls.
__device__ __forceinline__ bool row_valid(const uint8_t* validity, int64_t r) {
  return !validity || ((validity[r >> 3] >> (r & 7)) & 1);
}

// The raw bits of row r of a fixed-width column, zero-extended; a BOOL column's bit.
__device__ __forceinline__ uint64_t load_fixed_raw(int32_t type, const void* values, int64_t r) {
  uint64_t raw;
  switch (type) {
    case QE_TYPE_INT64:
    case QE_TYPE_FLOAT64: raw = ((const uint64_t*)values)[r]; break;
    case QE_TYPE_INT32:
    case QE_TYPE_DATE32: raw = ((const uint32_t*)values)[r]; break;
    case QE_TYPE_UINT8: raw = ((const uint8_t*)values)[r]; break;
    default: raw = (((const uint8_t*)values)[r >> 3] >> (r & 7)) & 1; break;  // BOOL
  }
  return raw;
}

// A wave's 64 result bits -> the two 32-bit words of rows [64 c, 64 c + 64) (bitmaps hold nwords words).
__device__ __forceinline__ void store_bits64(uint32_t* __restrict__ bm, int64_t c, int64_t nwords, uint64_t bits, int lane) {
  if (lane == 0 && 2 * c < nwords) bm[2 * c] = (uint32_t)bits;
  if (lane == 1 && 2 * c + 1 < nwords) bm[2 * c + 1] = (uint32_t)(bits >> 32);
}

struct Blocks {  // working memory of one call: freed stream-ordered when the call returns
  qe_ctx* ctx;
  std::vector<void*> ps;
  explicit Blocks(qe_ctx* c) : ctx(c) {}
  Blocks(const Blocks&) = delete;
  Blocks& operator=(const Blocks&) = delete;
  ~Blocks() {
    for (void* p : ps) dev_free(ctx, p);
  }
  int alloc(size_t bytes, void** out) {
    QE_TRY(dev_alloc(ctx, bytes ? bytes : 8, out));
    ps.push_back(*out);
    return QE_OK;
  }
  void keep(void* p) { ps.erase(std::find(ps.begin(), ps.end(), p)); }  // the caller owns it from here
};

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Workgroups of a grid-stride kernel over n elements: one element per thread, at most 8 per CU.
inline int stride_grid(const qe_ctx* ctx, int64_t n, int threads = 256) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)div_up((uint64_t)n, threads), (int64_t)ctx->num_cus * 8));
}

}  // namespace qe
