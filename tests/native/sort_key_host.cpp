// Host driver for query-engines_amd/csrc/qe_sort_key.hpp (plain g++): reads lines
//   <type> <flags> <valid 0|1> <raw value bits, hex>
// and prints, per line, "<null bit> <value field, hex>" as the sort kernels would store them.
#include <cinttypes>
#include <cstdio>

#include "qe_sort_key.hpp"

int main() {
  int type, flags, valid;
  uint64_t raw;
  while (std::scanf("%d %d %d %" SCNx64, &type, &flags, &valid, &raw) == 4) {
    const int bits = qe::sort_value_bits(type);
    if (bits == 0) return 2;
    const uint64_t field = qe::sort_field(qe::sort_enc_fixed(type, raw), bits, valid != 0, flags);
    std::printf("%" PRIu64 " %016" PRIx64 "\n", qe::sort_null_bit(valid != 0, flags), field);
  }
  // sort_place: a 12-bit field at key bit 60 straddles words 0 and 1
  const uint64_t f = 0xABC;
  std::printf("place %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", qe::sort_place(f, 60, 0), qe::sort_place(f, 60, 1),
              qe::sort_place(f, 60, 2));
  return 0;
}
