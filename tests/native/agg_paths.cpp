// Host program (no GPU) over qe_agg_paths.hpp, for tests/test_agg_paths.py:
//   agg_paths ladder CUS JIT ROWS G1,G2,...  one line of JSON per (plan of agg_plans.hpp, expected groups): what
//                                         the first rung of the ladder that applies decides (knobs: the environment)
//   agg_paths geometry SEED COUNT         the sizing invariants over COUNT random tuples; prints the
//                                         violations, exit status 1 if there are any
//   agg_paths knobs                       the knob struct as the environment sets it
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>

#include "agg_plans.hpp"

using namespace qe;

static const char* path_name(int p) {
  static const char* n[] = {"regular", "compact", "compact_spill", "compact_twopass", "spill", "keyhash", "partition", "global"};
  return n[p];
}

static int ladder_plan(const char* name, const qe_column* cols, int ncols, const qe_pred_term* terms, int nterms,
                       const AggIn* aggs, int naggs, int cus, bool jit, int64_t rows, const char* groups) {
  Plan P;
  if (make_agg_plan(name, cols, ncols, terms, nterms, aggs, naggs, &P)) return 1;
  P.n = rows;
  int32_t acc[QE_MAX_AGGS];
  for (int j = 0; j < naggs; ++j) acc[j] = aggs[j].acc;
  const AggKnobs K = agg_knobs_now();
  const size_t budget = fused_lds_budget(K, jit, fused_block(0));
  for (const char* g = groups; g && *g; g = strchr(g, ',') ? strchr(g, ',') + 1 : nullptr) {
    const int64_t eg = atoll(g);
    // the state's table range (qe_hashagg_create_ex) and this plan's table in it (run_update)
    const LdsRange r = lds_table_range(eg, acc, naggs, !jit, budget);
    AggLadderIn in;
    in.jit = jit;
    in.num_cus = cus;
    in.expected_groups = eg;
    in.regular_bytes = lds_regular_layout(&P, naggs, r, !jit, budget);
    in.compact_ok = jit && compact_ok(P);
    in.compact_slot_bytes = in.compact_ok ? compact_slot_bytes(P) : 0;
    in.fused_budget = budget;
    in.pagg_budget = pagg_lds_budget(pagg_block());
    Plan S = P;
    auto table_bytes = [&](int log2) { return lds_table_layout(&S, naggs, log2, !jit); };
    const AggLadder L = agg_ladder(in, K, table_bytes);
    // the first rung that applies: its kernel source generates (try_rung) and a spilling pass
    // does not decline (spill_update)
    const AggCandidate* c = nullptr;
    PartLayout rec;
    int64_t buckets = 0;
    bool chunked = false, have_rec = false;
    for (int i = 0; i < L.n && !c; ++i) {
      const AggCandidate& x = L.c[i];
      Plan T = P;
      std::string src;
      size_t jl = 0;
      const bool spill = x.path == PATH_COMPACT_SPILL || x.path == PATH_SPILL;
      if (x.compact_slots) {
        T.lds_log2 = 16;
        T.lds_compact = x.compact_slots;
      }
      if (x.mp_n) T.mp_n = x.mp_n;
      if (x.path == PATH_SPILL || x.path == PATH_KEYHASH) lds_table_layout(&T, naggs, x.tlog2, !jit);
      if (x.path != PATH_REGULAR && x.path != PATH_PARTITION && x.path != PATH_GLOBAL && jit &&
          !gen_fused_source(T, T.lds_log2, &src, &jl, x.path == PATH_COMPACT_SPILL))
        continue;
      if (spill) {
        T.part_narrow = K.part_narrow ? 1 : 0;
        rec = part_layout(T);
        have_rec = true;
        if (!spill_sub_buckets(K, T.mp_n) || (uint64_t)rows * rec.bytes() > PART_REC_MAX_BYTES ||
            largest_table_log2(in.pagg_budget, table_bytes) < 8)
          continue;
      }
      if (x.path == PATH_PARTITION) {
        if (x.tlog2 < 8) continue;
        T.part_narrow = K.part_narrow && !part_soa() ? 1 : 0;
        lds_table_layout(&T, naggs, x.tlog2, !jit);
        const int log2p = part_buckets_log2(x.tlog2, eg, K.part_fast_fill ? pagg_fast_slots(T) : 0, K);
        const bool staged = part_staged_ok(T, log2p);
        rec = part_layout(T);
        have_rec = true;
        const PartGeometry G = part_geometry(rows, cus, log2p, staged, staged ? pscatter_block_for(log2p) : 512,
                                             (size_t)rec.bytes(), K);
        buckets = G.np;
        chunked = G.chunked;
      }
      c = &x;
    }
    printf("{\"plan\": \"%s\", \"groups\": %lld, \"path\": \"%s\", \"compact_slots\": %d, \"mp_n\": %d, \"sub_buckets\": %d, "
           "\"tlog2\": %d, \"buckets\": %lld, \"chunked\": %d, \"record_bytes\": %d, \"narrow\": %d, \"colmode\": %d}\n",
           name, (long long)eg, path_name(c->path), c->compact_slots, c->mp_n, c->sub_buckets, c->tlog2, (long long)buckets,
           (int)chunked, have_rec ? rec.bytes() : 0, have_rec ? (int)rec.narrow : 0, have_rec ? (int)rec.colmode : 0);
  }
  return 0;
}

// ---- geometry invariants ------------------------------------------------------------------------
static int bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      if (++bad <= 50) {             \
        printf("FAIL %s: ", #cond);  \
        printf(__VA_ARGS__);         \
        printf("\n");                \
      }                              \
    }                                \
  } while (0)

// the chunk table's regions in order, disjoint, aligned for their element types, inside the allocation
static void check_table(const ChunkTable& t, int64_t chunks, int64_t buckets, const char* what) {
  const size_t start[6] = {t.meta, t.sorted, t.prec, t.pcnt, t.pcur, t.pbase};
  const size_t len[6] = {(size_t)(1 + chunks) * 8, (size_t)chunks * 4, (size_t)buckets * 8,
                         (size_t)buckets * 4,      (size_t)buckets * 4, (size_t)buckets * 4};
  const size_t align[6] = {8, 4, 8, 4, 4, 4};
  for (int i = 0; i < 6; ++i) {
    EXPECT(start[i] % align[i] == 0, "%s region %d at %zu", what, i, start[i]);
    EXPECT(start[i] + len[i] <= (i < 5 ? start[i + 1] : t.bytes), "%s region %d [%zu, +%zu) chunks %lld buckets %lld", what, i,
           start[i], len[i], (long long)chunks, (long long)buckets);
  }
}

static int geometry(uint64_t seed, int count) {
  std::mt19937_64 rng(seed);
  auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  int forced_small = 0, n_chunked = 0;
  for (int i = 0; i < count; ++i) {
    // rows: every magnitude from 1 to 2^33, exact powers of two and their neighbours included
    const int mag = (int)pick(0, 33);
    int64_t rows = ((int64_t)1 << mag) + (pick(0, 3) == 0 ? pick(-1, 1) : pick(0, ((int64_t)1 << mag) - 1));
    if (rows < 1) rows = 1;
    const int cus = (int)pick(1, 304);
    const size_t rb = (size_t)pick(2, 40) * 4;  // 32-bit or 64-bit words
    AggKnobs K;
    K.part_chunked = (int)pick(-1, 1);
    K.part_wg_per_cu = (int)pick(1, 4);
    K.pagg_slices_per_cu = (int)pick(1, 16);
    K.spill_load = (int)pick(4, 7);
    {  // radix partition
      const int log2p = (int)pick(1, 13);
      const bool staged = pick(0, 3) != 0;
      const int sblock = staged ? (pick(0, 1) ? 1024 : 256) : 512;
      const PartGeometry G = part_geometry(rows, cus, log2p, staged, sblock, rb, K);
      const int64_t streams = G.g * G.np;
      EXPECT(G.g >= 1 && G.tw % 256 == 0 && G.g * G.tw >= rows && (G.g - 1) * G.tw < rows, "rows %lld g %lld tw %lld",
             (long long)rows, (long long)G.g, (long long)G.tw);
      EXPECT(G.open_slots == streams * PART_CH, "open slots");
      // every row in a full chunk plus one open chunk per stream, by either way of handing out ids
      EXPECT(G.cmax >= rows / PART_CH + streams, "cmax %lld rows %lld streams %lld", (long long)G.cmax, (long long)rows,
             (long long)streams);
      EXPECT(G.cmax >= G.g * (G.tw / PART_CH + G.np), "cmax %lld static ranges", (long long)G.cmax);
      EXPECT(!G.chunked || (staged && K.part_chunked != 0 && G.np <= CHUNK_PLAN_MAXB), "chunked without its conditions");
      EXPECT(!G.chunked || K.part_chunked == 1 || G.open_slots <= rows, "auto chunked: open %lld rows %lld",
             (long long)G.open_slots, (long long)rows);
      if (G.chunked) {
        ++n_chunked;
        check_table(G.table, G.cmax, G.np, "partition");
        EXPECT(G.rec_slots == G.cmax * PART_CH, "record slots");
        EXPECT(G.rec_bytes >= (size_t)G.cmax * PART_CH * rb && G.rec_bytes <= PART_REC_MAX_BYTES, "record bytes %zu", G.rec_bytes);
        EXPECT(G.max_slices >= G.tmax + G.np && G.slice_bytes >= (size_t)(2 + 2 * G.max_slices) * 8, "slices");
        // forced: the open chunks within 4x the rows, down to the one workgroup the scatter needs
        if (K.part_chunked == 1) {
          if (4 * rows >= G.np * PART_CH) {
            EXPECT(G.open_slots <= 4 * rows, "forced chunked: open %lld rows %lld g %lld np %lld", (long long)G.open_slots,
                   (long long)rows, (long long)G.g, (long long)G.np);
          } else {
            ++forced_small;
            EXPECT(G.g == 1, "forced chunked below one workgroup's chunks: g %lld", (long long)G.g);
          }
        }
      } else {
        EXPECT(G.count_bytes >= (2 * (size_t)streams + 1) * 8 && G.cells == (size_t)streams, "counts");
      }
      const int64_t R = pick(0, rows);
      const CountedSlices S = counted_slices(R, G.np, cus);
      // k_part_slices cuts each bucket's records into slices of cw: at most one partial slice per bucket
      EXPECT(S.cw >= 256 && S.max_slices >= G.np + R / S.cw && S.slice_bytes >= (size_t)(2 + 2 * S.max_slices) * 8,
             "counted slices R %lld cw %lld", (long long)R, (long long)S.cw);
    }
    {  // spilling pass
      const int SB = 1 << (int)pick(0, 3), bpc = (int)pick(0, 8);
      const int sblock = pick(0, 1) ? 1024 : 512;
      const int64_t kept = pick(512, 65536), eg = pick(1, 1 << 22);
      const SpillGeometry G = spill_geometry(rows, cus, bpc, sblock, SB, rb, kept, eg, K);
      const int64_t streams = (int64_t)G.sgrid * (sblock / 64) * SB;
      EXPECT(G.sgrid >= 1 && G.sgrid <= cus * std::max(1, bpc), "sgrid %d", G.sgrid);
      EXPECT(G.cmax >= rows / PART_CH + streams, "spill cmax %lld rows %lld streams %lld", (long long)G.cmax, (long long)rows,
             (long long)streams);
      check_table(G.table, G.cmax, SB, "spill");
      EXPECT(G.rec_slots == G.cmax * PART_CH && G.rec_bytes >= (size_t)G.cmax * PART_CH * rb, "spill records");
      EXPECT(G.slice_bytes >= (size_t)(2 + 2 * (G.tmax + SB)) * 8, "spill slices");
      EXPECT(G.mp_keep <= (1ull << 32), "mp_keep %llu", (unsigned long long)G.mp_keep);
      EXPECT((eg > kept * K.spill_load / 8) == (G.mp_keep < (1ull << 32)), "kept share: eg %lld kept %lld keep %llu", (long long)eg,
             (long long)kept, (unsigned long long)G.mp_keep);
    }
  }
  printf("{\"tuples\": %d, \"chunked\": %d, \"forced_below_one_workgroup\": %d, \"violations\": %d}\n", count, n_chunked,
         forced_small, bad);
  return bad ? 1 : 0;
}

static int knobs() {
  const AggKnobs K = agg_knobs_now();
  printf("{\"lds_compact\": %d, \"mp_spill\": %d, \"part_chunked\": %d, \"spill_load\": %d, \"compact_load\": %d, "
         "\"compact_spill\": %d, \"compact_twopass\": %d, \"spill_maxpct\": %d, \"spill_subbuckets\": %d, \"mp_max\": %d, "
         "\"lds_budget_kb\": %d, \"part_narrow\": %d, \"part_fill_shift\": %d, \"part_fast_fill\": %d, \"part_wg_per_cu\": %d, "
         "\"pagg_slices_per_cu\": %d, \"fused_wg_per_cu\": %d, \"nn_implicit\": %d}\n",
         K.lds_compact, K.mp_spill, K.part_chunked, K.spill_load, K.compact_load, K.compact_spill, K.compact_twopass,
         K.spill_maxpct, K.spill_subbuckets, K.mp_max, K.lds_budget_kb, K.part_narrow, K.part_fill_shift, K.part_fast_fill,
         K.part_wg_per_cu, K.pagg_slices_per_cu, K.fused_wg_per_cu, K.nn_implicit);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "ladder")) {
    const int cus = atoi(argv[2]);
    const bool jit = atoi(argv[3]) != 0;
    const int64_t rows = atoll(argv[4]);
    return for_each_agg_plan([&](const char* name, const qe_column* c, int nc, const qe_pred_term* t, int nt, const AggIn* a,
                                 int na, int) { return ladder_plan(name, c, nc, t, nt, a, na, cus, jit, rows, argv[5]); });
  }
  if (argc >= 4 && !strcmp(argv[1], "geometry")) return geometry(strtoull(argv[2], nullptr, 10), atoi(argv[3]));
  if (argc >= 2 && !strcmp(argv[1], "knobs")) return knobs();
  return 2;
}
