// Host driver for query-engines_amd/csrc/qe_topk_plan.hpp (plain g++): reads lines
//   p <need> <m> <bin> <count> ... (m pairs)          -> "<bin> <below> <tied>" (threshold-bin pick; other bins 0)
//   d <rows> <m> <digit> <bin> <count> ... (m triples) -> "<digit>" (highest varying digit of a word, -1: none)
//   s <candidates> <k> <small_max>                     -> "1" / "0" (stop rule)
//   a <n> <k> <small_max>                              -> "1" / "0" (QE_TOPK_AUTO selects)
//   t <k> <tied> <m> <below> <tied> ... (m pairs)      -> "<need> <candidates>" before, after each pick, after the cut
// and ends with the header's constants.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "qe_topk_plan.hpp"

int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'p') {
      int64_t need;
      int m;
      if (std::scanf("%" SCNd64 " %d", &need, &m) != 2) return 2;
      std::vector<uint32_t> hist(256, 0);
      for (int i = 0; i < m; ++i) {
        int b;
        uint32_t c;
        if (std::scanf("%d %" SCNu32, &b, &c) != 2 || b < 0 || b > 255) return 2;
        hist[b] = c;
      }
      const qe::TopkPick P = qe::topk_pick_bin(hist.data(), need);
      std::printf("%d %" PRId64 " %" PRId64 "\n", P.bin, P.below, P.tied);
    } else if (op == 'd') {
      int64_t rows;
      int m;
      if (std::scanf("%" SCNd64 " %d", &rows, &m) != 2) return 2;
      std::vector<uint32_t> hist(8 * 256, 0);
      for (int i = 0; i < m; ++i) {
        int g, b;
        uint32_t c;
        if (std::scanf("%d %d %" SCNu32, &g, &b, &c) != 3 || g < 0 || g > 7 || b < 0 || b > 255) return 2;
        hist[256 * g + b] = c;
      }
      std::printf("%d\n", qe::topk_top_digit(hist.data(), rows));
    } else if (op == 's') {
      int64_t c, k, s;
      if (std::scanf("%" SCNd64 " %" SCNd64 " %" SCNd64, &c, &k, &s) != 3) return 2;
      std::printf("%d\n", qe::topk_stop(c, k, s) ? 1 : 0);
    } else if (op == 'a') {
      int64_t n, k, s;
      if (std::scanf("%" SCNd64 " %" SCNd64 " %" SCNd64, &n, &k, &s) != 3) return 2;
      std::printf("%d\n", qe::topk_use_select(n, k, s) ? 1 : 0);
    } else if (op == 't') {
      int64_t k, tied;
      int m;
      if (std::scanf("%" SCNd64 " %" SCNd64 " %d", &k, &tied, &m) != 3) return 2;
      qe::TopkNeed C{k, 0, tied};
      std::printf("%" PRId64 " %" PRId64, C.need(), C.candidates());
      for (int i = 0; i < m; ++i) {
        qe::TopkPick P{0, 0, 0};
        if (std::scanf("%" SCNd64 " %" SCNd64, &P.below, &P.tied) != 2) return 2;
        C.take(P);
        std::printf(" %" PRId64 " %" PRId64, C.need(), C.candidates());
      }
      C.cut();
      std::printf(" %" PRId64 " %" PRId64 "\n", C.need(), C.candidates());
    } else {
      return 2;
    }
  }
  std::printf("const %d %d\n", (int)QE_TOPK_STOP_FACTOR, (int)QE_TOPK_AUTO_DIV);
  return 0;
}
