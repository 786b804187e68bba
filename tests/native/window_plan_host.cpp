// Host driver for query-engines_amd/csrc/qe_window_plan.hpp (plain g++): reads lines
//   c <fn> <frame> <input type> <offset>      -> "<status> <output type> <takes input> <nullable>"
//   s <m> <fn> <input> ... (m pairs)           -> "<scans> <kind> <input> ... (per scan) <scan of fn> ... (m)"
//   b <n> <scans> <functions>                  -> "<working-memory bytes>"
// and ends with the header's constants.
#include <cinttypes>
#include <cstdio>

#include "qe_window_plan.hpp"

int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'c') {
      int32_t fn, frame, type, out;
      int64_t offset;
      if (std::scanf("%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd64, &fn, &frame, &type, &offset) != 4) return 2;
      const int st = qe::window_check(fn, frame, type, offset, &out);
      std::printf("%d %d %d %d\n", st, (int)out, qe::window_fn_known(fn) && qe::window_takes_input(fn) ? 1 : 0,
                  qe::window_fn_known(fn) && qe::window_nullable(fn) ? 1 : 0);
    } else if (op == 's') {
      int m;
      if (std::scanf("%d", &m) != 1 || m < 0 || m > QE_MAX_AGGS) return 2;
      qe_window_fn fns[QE_MAX_AGGS] = {};
      for (int i = 0; i < m; ++i)
        if (std::scanf("%" SCNd32 " %" SCNd32, &fns[i].fn, &fns[i].input) != 2) return 2;
      const qe::WindowScans S = qe::window_scans(fns, m);
      std::printf("%d", (int)S.n);
      for (int j = 0; j < S.n; ++j) std::printf(" %d %d", (int)S.kind[j], (int)S.input[j]);
      for (int i = 0; i < m; ++i) std::printf(" %d", (int)S.of_fn[i]);
      std::printf("\n");
    } else if (op == 'b') {
      int64_t n;
      int32_t scans, fns;
      if (std::scanf("%" SCNd64 " %" SCNd32 " %" SCNd32, &n, &scans, &fns) != 3) return 2;
      std::printf("%" PRId64 "\n", qe::window_work_bytes(n, scans, fns));
    } else {
      return 2;
    }
  }
  std::printf("const %d %d %d\n", (int)qe::WIN_TILE, (int)qe::WIN_SMALL_MAX, (int)QE_MAX_AGGS);
  return 0;
}
