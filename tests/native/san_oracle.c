/* TEST INFRASTRUCTURE (SURVEY §5 sanitizers): the oracle's C restatement (oracle/cpu_baseline.c)
 * under AddressSanitizer + UBSan, multi-threaded. Prints "key sum count min max" per group in key
 * order; tests/test_sanitizers.py compares with the Python oracle. qe_cpu_c4_mod runs beside it
 * (exit status 3 on a difference): the same moduli must give the same groups, and 40-bit values
 * over 6500 keys (the growing hash map) the same groups at any thread count. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../oracle/cpu_baseline.c"

static int by_key(const void* x, const void* y) {
  const qe_group_out *a = (const qe_group_out*)x, *b = (const qe_group_out*)y;
  return (a->key > b->key) - (a->key < b->key);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int64_t row0 = atoll(argv[1]), rows = atoll(argv[2]);
  const int threads = atoi(argv[3]);
  qe_group_out* out = (qe_group_out*)calloc(2048, sizeof(qe_group_out));
  int64_t ng = 0;
  qe_cpu_c4(row0, rows, 42, threads, 1 << 19, 1024, out, 2048, &ng);
  qsort(out, (size_t)ng, sizeof(qe_group_out), by_key);
  {
    qe_group_out* o2 = (qe_group_out*)calloc(2048, sizeof(qe_group_out));
    int64_t n2 = 0;
    qe_cpu_c4_mod(row0, rows, 42, threads, 1 << 19, 1024, 1ll << 20, 1ll << 20, o2, 2048, &n2);
    qsort(o2, (size_t)(n2 < 2048 ? n2 : 2048), sizeof(qe_group_out), by_key);
    const int same = n2 == ng && memcmp(out, o2, (size_t)ng * sizeof(qe_group_out)) == 0;
    free(o2);
    if (!same) return 3;
    qe_group_out* w1 = (qe_group_out*)calloc(8192, sizeof(qe_group_out));
    qe_group_out* wt = (qe_group_out*)calloc(8192, sizeof(qe_group_out));
    int64_t m1 = 0, mt = 0;
    qe_cpu_c4_mod(row0, rows, 42, 1, 1ll << 36, 6500, 1ll << 40, 1ll << 40, w1, 8192, &m1);
    qe_cpu_c4_mod(row0, rows, 42, threads, 1ll << 36, 6500, 1ll << 40, 1ll << 40, wt, 8192, &mt);
    qsort(w1, (size_t)(m1 < 8192 ? m1 : 8192), sizeof(qe_group_out), by_key);
    qsort(wt, (size_t)(mt < 8192 ? mt : 8192), sizeof(qe_group_out), by_key);
    const int wsame = m1 == mt && m1 <= 6500 && memcmp(w1, wt, (size_t)m1 * sizeof(qe_group_out)) == 0;
    free(w1);
    free(wt);
    if (!wsame) return 3;
  }
  for (int64_t i = 0; i < ng; ++i)
    printf("%lld %lld %lld %lld %lld\n", (long long)out[i].key, (long long)out[i].sum, (long long)out[i].count,
           (long long)out[i].min, (long long)out[i].max);
  free(out);
  return 0;
}
