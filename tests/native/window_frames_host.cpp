// Host driver for the rules qe_window_plan.hpp adds for qe_window_eval_frames (plain g++): reads lines
//   c <fn> <frame> <input type> <offset> <has bounds> <lo> <hi>
//        -> "<status> <output type> <takes input> <nullable> <lo clamped to 2^31-1 rows> <hi clamped>"
//   k <bound> <n>                                   -> "<the bound clamped to [-n, n]>"
//   s <n> <m> <fn> <frame> <input> <lo> <hi> ... (m functions)
//        -> "<scans> <kind> <input> <backward> <block> ... (per scan) <forward scan of fn> ... (m) <backward scan of fn> ... (m)"
//   b <n> <m> <fn> <frame> <input> <lo> <hi> ... (m functions)
//        -> "<working-memory bytes> <window_work_bytes with window_scans' count of scans (what qe_window_eval sized)>"
// and ends with the header's constants.
#include <cinttypes>
#include <cstdio>

#include "qe_window_plan.hpp"

static bool read_fns(int64_t* n, int* m, qe_window_fn* fns, qe_window_bounds* bounds) {
  if (std::scanf("%" SCNd64 " %d", n, m) != 2 || *m < 0 || *m > QE_MAX_AGGS) return false;
  for (int i = 0; i < *m; ++i)
    if (std::scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd64, &fns[i].fn, &fns[i].frame, &fns[i].input, &bounds[i].lo,
                   &bounds[i].hi) != 5)
      return false;
  return true;
}

int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    qe_window_fn fns[QE_MAX_AGGS] = {};
    qe_window_bounds bounds[QE_MAX_AGGS] = {};
    int64_t n;
    int m;
    if (op == 'c') {
      int32_t fn, frame, type, out, has;
      int64_t offset, lo, hi;
      if (std::scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd32 " %" SCNd64 " %" SCNd64, &fn, &frame, &type, &offset,
                     &has, &lo, &hi) != 7)
        return 2;
      const int st = qe::window_frames_check(fn, frame, type, offset, has != 0, &out);
      const bool known = qe::window_frames_fn_known(fn);
      std::printf("%d %d %d %d %" PRId64 " %" PRId64 "\n", st, (int)out, known && qe::window_frames_takes_input(fn) ? 1 : 0,
                  known && qe::window_frames_nullable(fn) ? 1 : 0, qe::window_clamp_bound(lo, INT32_MAX),
                  qe::window_clamp_bound(hi, INT32_MAX));
    } else if (op == 'k') {
      int64_t b;
      if (std::scanf("%" SCNd64 " %" SCNd64, &b, &n) != 2) return 2;
      std::printf("%" PRId64 "\n", qe::window_clamp_bound(b, n));
    } else if (op == 's') {
      if (!read_fns(&n, &m, fns, bounds)) return 2;
      const qe::WindowFrameScans S = qe::window_frame_scans(fns, bounds, m, n);
      std::printf("%d", (int)S.n);
      for (int j = 0; j < S.n; ++j) std::printf(" %d %d %d %" PRId64, (int)S.kind[j], (int)S.input[j], (int)S.back[j], S.block[j]);
      for (int i = 0; i < m; ++i) std::printf(" %d", (int)S.fwd_of_fn[i]);
      for (int i = 0; i < m; ++i) std::printf(" %d", (int)S.bwd_of_fn[i]);
      std::printf("\n");
    } else if (op == 'b') {
      if (!read_fns(&n, &m, fns, bounds)) return 2;
      std::printf("%" PRId64 " %" PRId64 "\n", qe::window_frames_work_bytes(n, fns, bounds, m),
                  qe::window_work_bytes(n, qe::window_scans(fns, m).n, m));
    } else {
      return 2;
    }
  }
  std::printf("const %d %d %d\n", (int)qe::WIN_TILE, (int)qe::WIN_SMALL_MAX, (int)QE_MAX_AGGS);
  return 0;
}
