// Host driver for query-engines_amd/csrc/qe_join_plan.hpp (plain g++): reads lines
//   w <type> <raw value bits, hex>     -> "<key word, hex>"
//   c <build type> <probe type>        -> "1" / "0" (do the types join)
//   s <non-null build rows>            -> "<slots>"
//   h <key word, hex> <slots>          -> "<home slot>"
// and ends with the header's constants.
#include <cinttypes>
#include <cstdio>

#include "qe_join_plan.hpp"

int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    if (op == 'w') {
      int type;
      uint64_t raw;
      if (std::scanf("%d %" SCNx64, &type, &raw) != 2 || !qe::join_key_type(type)) return 2;
      std::printf("%016" PRIx64 "\n", qe::join_key_word(type, raw));
    } else if (op == 'c') {
      int a, b;
      if (std::scanf("%d %d", &a, &b) != 2) return 2;
      std::printf("%d\n", qe::join_compatible(a, b) ? 1 : 0);
    } else if (op == 's') {
      int64_t rows;
      if (std::scanf("%" SCNd64, &rows) != 1) return 2;
      std::printf("%" PRId64 "\n", qe::join_slots(rows));
    } else if (op == 'h') {
      uint64_t word, slots;
      if (std::scanf("%" SCNx64 " %" SCNu64, &word, &slots) != 2) return 2;
      std::printf("%" PRIu64 "\n", qe::join_home(word, slots));
    } else {
      return 2;
    }
  }
  std::printf("const %016" PRIx64 " %016" PRIx64 " %" PRId64 " %" PRId64 "\n", qe::JOIN_EMPTY_WORD, qe::JOIN_CANON_NAN,
              qe::JOIN_MIN_SLOTS, qe::JOIN_MAX_ROWS);
  return 0;
}
