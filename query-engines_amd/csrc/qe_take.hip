// Gather by row index: what applies a sort's, a join's or a window's row indices.
//
// qe_take
//   k_take: one row per lane, validity / BOOL words built per wave with __ballot; UTF8 through the
//   (start, length) pairs, length scan and byte copy of qe_filter.hip.
// qe_take_or_null
//   k_take<true>: index -1 is "no row" and gives a null row (the build side of a LEFT join).
#include "qe_rows.hpp"

namespace qe {

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
        const bool b = ok && load_fixed_raw(QE_TYPE_BOOL, C.in, r);
        store_bits64((uint32_t*)C.out, c, nwords, __ballot(b), lane);
      }
      if (C.out_valid) {
        const bool v = ok && row_valid(C.in_valid, r);
        store_bits64(C.out_valid, c, nwords, __ballot(v), lane);
      }
    }
  }
}

}  // namespace qe

using namespace qe;

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
  Blocks blk(ctx);
  char* base;
  QE_TRY(blk.alloc(256 + (size_t)nutf8 * (pairs_b + tsum_b), (void**)&base));
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
    const int grid = stride_grid(ctx, m);
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
