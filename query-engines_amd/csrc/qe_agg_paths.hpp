// qe_agg_paths.hpp — which GROUP BY path an update takes and how large its buffers
// are, as host functions of plain numbers: no HIP calls, no allocation, nothing read from a state.
// qe_hashagg.hip's run_update / partition_rows / spill_update ask these and then only allocate,
// clear and launch; tests/native/agg_paths.cpp runs them on a CPU (tests/test_agg_paths.py).
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "qe_dev.hpp"

namespace qe {

constexpr size_t HA_LDS_BUDGET = 80 * 1024;         // bytes of LDS per workgroup (2 workgroups / CU)
constexpr size_t HA_LDS_BUDGET_1024 = 152 * 1024;   // ... of a 1024-thread workgroup (one per CU)
constexpr int CHUNK_PLAN_MAXB = 512;                // buckets of the staged scatter
constexpr uint64_t PART_REC_MAX_BYTES = 96ull << 30;  // most record bytes of a chunked update
constexpr uint64_t PART_OVF_RECORDS = 1ull << 20;   // overflow records of a record aggregation pass
// Exact fp64 SUM in the specialised kernels' LDS tables: the 192-bit carry window through the per-wave
// queue. LDS words per slot beyond acc.
inline int fx_window_idx_words() { return 2; }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- knobs ------------------------------------------------------------------------------------
// Every QE_* value the path choice and the sizing read. Out-of-range values: some knobs fall back
// to a default, some clamp (as each always did; see the reader).
struct AggKnobs {
  // read per call (tests switch them between the updates of one process)
  bool lds_compact = true;  // QE_LDS_COMPACT=0: never the compact table
  bool mp_spill = true;     // QE_MP_SPILL=0: no spilling pass (fused key-hash passes instead)
  int part_chunked = -1;    // QE_PART_CHUNKED: 0 never, 1 whenever the scatter is staged, unset (-1): by rule
  int spill_load = 6;       // QE_SPILL_LOAD: kept share of the spilling pass in eighths of the kept table's slots, 4..7
  // read once per process
  int compact_load = 98;         // QE_COMPACT_LOAD: percent, 50..99
  bool compact_spill = true;     // QE_COMPACT_SPILL=0: off
  bool compact_twopass = false;  // QE_COMPACT_TWOPASS=1: opt-in
  int spill_maxpct = 70;         // QE_SPILL_MAXPCT: percent, 10..90; anything else 0 = round 4's rule
  int spill_subbuckets = 2;      // QE_SPILL_SUBBUCKETS: the most, 1, 2 or 4
  int mp_max = 2;                // QE_MP_MAX: most bucket passes before partitioning, 2..8
  int lds_budget_kb = 0;         // QE_LDS_BUDGET_KB: 16..156; 0 = by kernel (fused_lds_budget)
  bool part_narrow = true;       // QE_PART_NARROW=0: 64-bit partition records
  int part_fill_shift = 0;       // QE_PART_FILL_SHIFT: 1..3; 0 = by rule (part_buckets_log2)
  int part_fast_fill = 0;        // QE_PART_FAST_FILL: percent, 10..90; 0 = off
  int part_wg_per_cu = 2;        // QE_PART_WG_PER_CU: count / scatter workgroups per CU, 1..32
  int pagg_slices_per_cu = 8;    // QE_PAGG_SLICES_PER_CU: 1..64
  int fused_wg_per_cu = 0;       // QE_FUSED_WG_PER_CU: fused workgroups per CU (>= 1); 0 = the state's
  bool nn_implicit = true;       // QE_NN_IMPLICIT=0: always store the non-null counts (A/B and debugging)
};

inline char knob_char(const char* name) {  // first character, 0 when unset or empty
  const char* e = getenv(name);
  return e ? e[0] : 0;
}
inline int knob_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : unset;
}
inline int knob_in(const char* name, int unset, int lo, int hi, int fallback) {  // out of range: the fallback
  const int v = knob_int(name, unset);
  return v >= lo && v <= hi ? v : fallback;
}
inline int knob_clamped(const char* name, int unset, int lo, int hi) {  // out of range: the nearest bound
  const char* e = getenv(name);
  return e && *e ? std::max(lo, std::min(hi, atoi(e))) : unset;
}

inline void read_agg_knobs(AggKnobs& k, bool per_call) {
  if (per_call) {
    k.lds_compact = knob_char("QE_LDS_COMPACT") != '0';
    k.mp_spill = knob_char("QE_MP_SPILL") != '0';
    const char c = knob_char("QE_PART_CHUNKED");
    k.part_chunked = c ? (c == '0' ? 0 : 1) : -1;
    k.spill_load = knob_clamped("QE_SPILL_LOAD", 6, 4, 7);
    return;
  }
  k.compact_load = knob_in("QE_COMPACT_LOAD", 98, 50, 99, 98);
  k.compact_spill = knob_char("QE_COMPACT_SPILL") != '0';
  k.compact_twopass = knob_char("QE_COMPACT_TWOPASS") == '1';
  k.spill_maxpct = knob_in("QE_SPILL_MAXPCT", 70, 10, 90, 0);
  const int sb = knob_int("QE_SPILL_SUBBUCKETS", 2);
  k.spill_subbuckets = sb == 1 || sb == 2 || sb == 4 ? sb : 2;
  k.mp_max = knob_clamped("QE_MP_MAX", 2, 2, 8);
  k.lds_budget_kb = knob_clamped("QE_LDS_BUDGET_KB", 0, 16, 156);
  k.part_narrow = knob_char("QE_PART_NARROW") != '0';
  k.part_fill_shift = knob_in("QE_PART_FILL_SHIFT", 0, 1, 3, 0);
  k.part_fast_fill = knob_in("QE_PART_FAST_FILL", 0, 10, 90, 0);
  k.part_wg_per_cu = knob_in("QE_PART_WG_PER_CU", 2, 1, 32, 2);
  k.pagg_slices_per_cu = knob_in("QE_PAGG_SLICES_PER_CU", 8, 1, 64, 8);
  k.fused_wg_per_cu = knob_clamped("QE_FUSED_WG_PER_CU", 0, 1, 1 << 30);
  k.nn_implicit = knob_char("QE_NN_IMPLICIT") != '0';
}
// The once-per-process knobs (the per-call ones at their defaults: no getenv after the first use).
inline const AggKnobs& agg_knobs() {
  static const AggKnobs k = [] {
    AggKnobs v;
    read_agg_knobs(v, false);
    return v;
  }();
  return k;
}
inline AggKnobs agg_knobs_now() {  // ... with the per-call knobs as the environment has them now
  AggKnobs k = agg_knobs();
  read_agg_knobs(k, true);
  return k;
}

// ---- LDS tables ---------------------------------------------------------------------------------
// LDS layout for a table of 2^log2 slots under this launch's aggregates. Returns bytes.
// LDS words per slot beyond acc of an aggregate with idx arrays: fp64 MIN / MAX keep 4 row
// indices; an exact fp64 SUM keeps 4 more words (256-bit + status) in the generic kernel, and in
// the plan-specialised kernels 5 (limb window, qe_dev.hpp fxl_add) or 2 (192-bit window, fxw_add);
// rare rows go global.
inline size_t idx_words(int acc, bool generic) { return acc == ACC_SUM_X && !generic ? (size_t)fx_window_idx_words() : 4; }

inline size_t lds_table_layout(Plan* P, int naggs, int log2, bool generic) {
  const size_t SS = ((size_t)1 << log2) + 2;
  size_t off = 8 * SS;  // keys
  P->off_cstar = (int32_t)off;
  off += 4 * SS;
  off = (off + 15) & ~size_t(15);
  for (int j = 0; j < naggs; ++j) {
    const DAgg& a = P->aggs[j];
    if (!generic && a.share) continue;  // the specialised kernels read the shared accumulator
    if (a.acc != ACC_NONE) {
      P->off_acc[j] = (int32_t)off;
      off += 8 * SS;
    }
    if (a.track_nn) {
      P->off_nn[j] = (int32_t)off;
      off += 4 * SS;
      off = (off + 15) & ~size_t(15);
    }
    if (acc_has_idx(a.acc)) {
      P->off_idx[j] = (int32_t)off;
      off += 8 * idx_words(a.acc, generic) * SS;
    }
  }
  P->lds_log2 = log2;
  return off;
}

// LDS bytes with no nullable inputs (the smallest layout a launch can have).
inline size_t lds_bytes_min(const int32_t* acc, int naggs, int log2, bool generic) {
  const size_t SS = ((size_t)1 << log2) + 2;
  size_t b = 12 * SS + 16;
  for (int j = 0; j < naggs; ++j) {
    if (acc[j] != ACC_NONE) b += 8 * SS;
    if (acc_has_idx(acc[j])) b += 8 * idx_words(acc[j], generic) * SS;
  }
  return b;
}

// LDS bytes a workgroup's table may take. The generic kernel runs two 512-thread workgroups per
// CU (80 KiB each). The specialised kernel's 1024-thread workgroups run one per CU, so its table
// may take nearly all of the CU's 160 KiB: twice the groups in one pass (C4 shape: up to ~2.5K
// groups in a 4096-slot table instead of ~1.3K in 2048 slots). QE_LDS_BUDGET_KB overrides.
inline size_t fused_lds_budget(const AggKnobs& K, bool jit, int fused_block0) {
  if (K.lds_budget_kb) return (size_t)K.lds_budget_kb * 1024;
  return jit && fused_block0 == 1024 ? HA_LDS_BUDGET_1024 : HA_LDS_BUDGET;
}
// ... and the table of the aggregation pass over partition / spill records (qe_pagg)
inline size_t pagg_lds_budget(int pagg_block) { return pagg_block == 1024 ? HA_LDS_BUDGET_1024 : HA_LDS_BUDGET; }

// A state's LDS table range, fixed at create: 2x the expected groups (load factor <= 0.5); a launch
// may shrink it down to 1.25x (log2_min) to fit the per-workgroup budget, else the launch is
// global-only (log2 = 0).
struct LdsRange {
  int log2 = 0, log2_min = 0;
};
inline LdsRange lds_table_range(int64_t expected_groups, const int32_t* acc, int naggs, bool generic, size_t budget) {
  LdsRange r;
  int log2 = 8;
  r.log2_min = 8;
  while (log2 < 16 && ((int64_t)1 << log2) < 2 * expected_groups) ++log2;
  while (r.log2_min < 16 && ((int64_t)1 << r.log2_min) < (5 * expected_groups + 3) / 4) ++r.log2_min;
  while (log2 > r.log2_min && lds_bytes_min(acc, naggs, log2, generic) > budget) --log2;
  r.log2 = lds_bytes_min(acc, naggs, log2, generic) <= budget ? log2 : 0;
  return r;
}

// Largest table of the state's range that fits the per-workgroup budget under this plan, P laid
// out for it; 0 bytes => global-only launch (the expected groups do not fit on chip).
inline size_t lds_regular_layout(Plan* P, int naggs, const LdsRange& r, bool generic, size_t budget) {
  if (r.log2 == 0) return 0;
  for (int log2 = r.log2; log2 >= r.log2_min; --log2) {
    const size_t b = lds_table_layout(P, naggs, log2, generic);
    if (b <= budget) return b;
  }
  P->lds_log2 = 0;
  return 0;
}

// log2 of the largest table of at most 2^16 slots whose bytes(log2) fit `budget`; below 8: none does.
template <typename Bytes>
inline int largest_table_log2(size_t budget, Bytes&& bytes) {
  int log2 = 16;
  while (log2 >= 8 && bytes(log2) > budget) --log2;
  return log2;
}

// Slots of the compact fused table (qe_jit.hip compact_*) in `budget` bytes of LDS, `reserve` of
// them the kernel's other state: 512, and 256 more for the spilling pass's chunk state (+2 special
// slots, 64 sinks).
inline int64_t compact_slots(size_t budget, size_t slot_bytes, size_t reserve) {
  return ((int64_t)((budget - reserve) / slot_bytes) - 66) & ~(int64_t)63;
}

// ---- the decision ladder ----------------------------------------------------------
enum AggPath : int {
  PATH_REGULAR = 0,      // one pass, the state's regular LDS table
  PATH_COMPACT,          // one pass, compact table
  PATH_COMPACT_SPILL,    // one spilling pass over a compact kept table + one record aggregation pass
  PATH_COMPACT_TWOPASS,  // two key-hash passes, compact table (opt-in)
  PATH_SPILL,            // two key-hash buckets: bucket 1 spilled as records (regular kept table)
  PATH_KEYHASH,          // mp_n fused passes over the columns, one key-hash bucket each
  PATH_PARTITION,        // radix partition, then record aggregation
  PATH_GLOBAL,           // global table only
};
// One rung: what it decides. A rung whose source generation or compile fails (or whose spilling
// pass declines) falls through to the next one of the list.
struct AggCandidate {
  int path = PATH_GLOBAL;
  int32_t compact_slots = 0;  // compact table slots (0: regular table)
  int mp_n = 0;               // key-hash buckets (spilling: 1 + sub-buckets)
  int sub_buckets = 0;        // sub-buckets of the spilled share
  int tlog2 = 0;              // log2 slots of the regular table the rung aggregates in (kept or record pass)
  uint64_t ovf_records = 0;   // overflow records it needs (0: the state's are enough)
};
struct AggLadder {
  int n = 0;
  AggCandidate c[8];
  void push(const AggCandidate& x) { c[n++] = x; }
};
struct AggLadderIn {
  bool jit = true;
  int num_cus = 256;
  int64_t expected_groups = 0;
  bool compact_off = false;  // the state gave the compact table up (a value did not fit)
  bool compact_ok = false;   // the plan shape takes the compact table (qe_jit.hip compact_ok)
  size_t regular_bytes = 0;  // LDS bytes of the state's regular table under this plan; 0: none fits
  size_t compact_slot_bytes = 0;
  size_t fused_budget = 0;   // fused_lds_budget
  size_t pagg_budget = 0;    // pagg_lds_budget
};

// table_bytes(k): LDS bytes of a regular table of 2^k slots under this plan (lds_table_layout).
template <typename Bytes>
inline AggLadder agg_ladder(const AggLadderIn& in, const AggKnobs& K, Bytes&& table_bytes) {
  AggLadder L;
  const int64_t eg = in.expected_groups;
  AggCandidate c;
  if (in.regular_bytes) {
    c.path = PATH_REGULAR;
    L.push(c);
    return L;
  }
  // Groups just past the regular LDS table: one pass with the compact table (qe_jit.hip
  // compact_*, 32-bit keys, <= 92 % load) when the plan shape and the expected groups allow it
  // (QE_LDS_COMPACT=0: never; read per call), before key-hash passes / spilling.
  if (in.jit && eg > 0 && !in.compact_off && K.lds_compact && in.compact_ok) {
    const int64_t nsl = compact_slots(in.fused_budget, in.compact_slot_bytes, 512);
    const uint64_t ovf = (uint64_t)in.num_cus * 8 * ((uint64_t)nsl + 2);
    // expected groups at most QE_COMPACT_LOAD percent of the slots (default 98; 1B rows, one box,
    // 6336 slots: 5,900 / 6,000 / 6,150 / 6,250 groups 4.04 / 4.02–4.15 / 4.24 / 4.97 ms in one pass
    // at 93–99 %, against 5.45–5.71 ms for the spilling pass; round 5: 5,400 / 5,700 groups 3.76 /
    // 3.87 ms at 88–92 %)
    if (nsl >= 512 && nsl * K.compact_load >= eg * 100) {
      c = AggCandidate{PATH_COMPACT, (int32_t)nsl, 0, 0, 0, ovf};
      L.push(c);
    }
    // Past the compact table (~5K groups for C4) and up to ~1.5 tables' worth: ONE spilling pass
    // whose kept share (key hashes below mp_keep, 6/8 of the compact table's slots) stays in the
    // compact table and whose other rows are written as records for one aggregation pass
    // (spill_update), instead of the 8-bucket partitioned path (QE_COMPACT_SPILL=0: off).
    const int64_t ksl = compact_slots(in.fused_budget, in.compact_slot_bytes, 512 + 256);  // (+ spill chunk state)
    // the spilled share goes through the regular aggregation table: at most half of it (1B rows:
    // 5,500 / 6,500 groups 5.95 / 6.59 ms against 8.23 / 8.25 partitioned; 8,192 groups, whose
    // ~3.4K spilled groups fill 84 % of a 4096-slot table, 11.0 against 8.1 ms)
    const int tl = largest_table_log2(in.pagg_budget, table_bytes);
    // QE_SPILL_MAXPCT (default 70): the spilled groups (expected groups beyond the kept share)
    // may fill this percentage of each sub-bucket's aggregation table; 0 = round 4's rule (kept
    // share counted at 3/4, half the table). 1B rows, one box, C4 shape, record-major spill at a
    // 6/8 kept share: 7,500 groups 5.97 ms, 8,192 groups in one spilled bucket (84 % of its table)
    // 6.82 ms, against 7.63 ms partitioned at 8,192; two sub-buckets reach ~10.5K groups (11,500
    // groups at 85 %: 8.63 ms, past the partitioned update's ~8.0). Round 5 (chunk-columnar spill
    // at 7/8): 7.04 ms at 7,000 groups, 8.71 at 8,192, so 60 % stopped at ~7.9K groups
    const int sp_pct = K.spill_maxpct;
    // the spilled share in SB sub-buckets (spill_hash's low bits), each aggregated by its own
    // slices: the fewest (1 or 2) whose aggregation tables stay within that percentage
    // (QE_SPILL_SUBBUCKETS: the most, 1, 2 or 4). 1B rows, one box: 8,192 groups 7.19 ms with
    // one spilled bucket, 7.07 with two (at 7,000 groups one: 6.24 against 6.55); 9,000 / 10,000
    // groups in two 7.28 / 7.66 ms, 12,000 / 16,000 in four 8.57 / 9.53, against 8.0–8.2 ms
    // partitioned on that box
    const int64_t kept_share = ksl * K.spill_load / 8, per_sb = ((int64_t)1 << tl) * sp_pct / 100;
    int sb = 1;
    while (sp_pct && sb < K.spill_subbuckets && eg - kept_share > sb * per_sb) sb *= 2;
    const int64_t spill_max = sp_pct ? kept_share + sb * per_sb : ksl * 3 / 4 + ((int64_t)1 << tl) / 2;
    if (K.compact_spill && ksl >= 512 && tl >= 8 && eg <= spill_max) {
      c = AggCandidate{PATH_COMPACT_SPILL, (int32_t)ksl, 1 + sb, sb, tl, (uint64_t)in.num_cus * 8 * ((uint64_t)ksl + 2)};
      L.push(c);
    }
    // Beyond the compact spill (~6.75K–10K groups for C4): two key-hash passes over the columns,
    // each keeping half the groups in the compact table (QE_COMPACT_TWOPASS=1, opt-in: 1B rows, one
    // box, 7,000 / 8,192 / 9,500 groups 8.02 / 8.17 / 9.09 ms against 7.78 / 7.81 / 7.96 ms for the
    // partitioned update — each pass's fuller compact table costs ~4 ms).
    if (K.compact_twopass && nsl >= 512 && eg <= nsl * 8 / 5) {
      c = AggCandidate{PATH_COMPACT_TWOPASS, (int32_t)nsl, 2, 0, 0, ovf};
      L.push(c);
    }
  }
  // Groups just beyond one LDS table: 2 passes of the fused kernel, each keeping one bucket of
  // key hashes, read the columns twice but write and re-read no records. Measured at 200M rows
  // (C4 shape): 2048 groups 1.86 ms in 2 passes against ~3.1 ms radix-partitioned; 3 passes lose
  // their edge (3000 groups 2.88 ms, 3800 groups 3.44 ms against 3.09 ms partitioned).
  // The generic kernel (JIT off, or no specialised kernel) passes too, with its own 80 KiB budget:
  // it has no partitioned path to fall back on, and global-only rows cost a device atomic each.
  if (eg > 0) {
    const int tlog2 = largest_table_log2(in.jit ? in.fused_budget : HA_LDS_BUDGET, table_bytes);
    const int64_t per_pass = (((int64_t)1 << tlog2) * 5) / 8;
    const int64_t np = tlog2 >= 8 ? (eg + per_pass - 1) / per_pass : 0;
    if (np >= 2 && np <= (in.jit ? K.mp_max : 8)) {
      // overflow records: a workgroup flushes at most its table's slots
      c = AggCandidate{PATH_KEYHASH, 0, (int)np, 0, tlog2, (uint64_t)in.num_cus * 8 * (((uint64_t)1 << tlog2) + 2)};
      // Two key-hash buckets (groups just beyond one LDS table; QE_MP_SPILL, read per call, 0 = two
      // fused passes): the spilling pass first (spill_update)
      if (np == 2 && in.jit) {
        AggCandidate s = c;
        s.path = PATH_SPILL;
        s.sub_buckets = 1;
        L.push(s);
      }
      L.push(c);
    }
  }
  // groups beyond the LDS table: radix-partition the selected rows by key hash first, then
  // aggregate record slices in LDS (the aggregation-pass table: the largest within its budget)
  if (in.jit && eg > 0) {
    c = AggCandidate{PATH_PARTITION, 0, 0, 0, largest_table_log2(in.pagg_budget, table_bytes), PART_OVF_RECORDS};
    L.push(c);
  }
  c = AggCandidate{};
  L.push(c);
  return L;
}

// ---- chunked records: the chunk table -----------------------------------------------------------
// One allocation (byte offsets): meta, qi64[1 + chunks]: [0] chunks claimed, then per chunk
// (bucket << 32 | records) | sorted, qi32[chunks]: chunk ids grouped by bucket | the planning
// counters of k_chunk_hist / k_chunk_slices / k_chunk_place per bucket: prec u64 (records), pcnt u32
// (chunks), pcur u32 (cursor), pbase u32.
struct ChunkTable {
  size_t meta = 0, sorted = 0, prec = 0, pcnt = 0, pcur = 0, pbase = 0, bytes = 0;
};
inline ChunkTable chunk_table(int64_t chunks, int64_t buckets) {
  ChunkTable t;
  t.sorted = (size_t)(1 + chunks) * 8;
  t.prec = (t.sorted + (size_t)chunks * 4 + 7) & ~(size_t)7;
  t.pcnt = t.prec + (size_t)buckets * 8;
  t.pcur = t.pcnt + (size_t)buckets * 4;
  t.pbase = t.pcur + (size_t)buckets * 4;
  t.bytes = t.pbase + (size_t)buckets * 4;
  return t;
}

// ---- radix partition (partition_rows) -----------------------------------------------------------
// buckets: about a quarter of the table's slots in groups per bucket while that takes <= 64
// buckets, half the slots beyond (a slice spans <= 2 buckets; QE_PART_FILL_SHIFT = 1 / 2 fixes
// half / a quarter). 1B rows, C4 shape, half-full against quarter-full tables: 65,536 groups
// 13.66 vs 13.50 ms, 262,144 14.87 vs 15.78, 1,048,576 (512 staged buckets instead of 1024
// direct) 19.1 vs 19.3, 4,194,304 20.9 vs 21.2, 16,777,216 27.6 vs 27.7.
// QE_PART_FAST_FILL (percent): buckets for the fast aggregation pass's own (larger) table of
// fast_slots, each bucket's expected groups at most that share of its slots (fewer buckets: longer
// scatter runs)
inline int part_buckets_log2(int tlog2, int64_t expected_groups, int64_t fast_slots, const AggKnobs& K) {
  auto fill = [&](int64_t per_bucket) {
    int l = 1;
    while (l < 13 && per_bucket * ((int64_t)1 << l) < expected_groups) ++l;
    return l;
  };
  const int64_t slots = (int64_t)1 << tlog2;
  if (K.part_fill_shift) return fill(slots >> K.part_fill_shift);
  int log2p = fill(slots >> 2);
  if (log2p > 6) log2p = fill(slots >> 1);
  const int64_t fs = K.part_fast_fill ? fast_slots * K.part_fast_fill / 100 : 0;
  return fs > 0 ? fill(fs) : log2p;
}

struct PartGeometry {
  int64_t np = 0;          // buckets
  int64_t g = 0;           // count / scatter workgroups
  int64_t tw = 0;          // rows per workgroup (a multiple of 256)
  int64_t open_slots = 0;  // record slots of one open chunk per (workgroup, bucket)
  int64_t cmax = 0;        // chunk ids
  bool chunked = false;
  // chunked only
  int64_t tmax = 0, max_slices = 0;  // aggregation slices: most over whole buckets, bound on all
  ChunkTable table;
  size_t rec_bytes = 0, slice_bytes = 0;
  int64_t rec_slots = 0;  // cmax * PART_CH: what the aggregation pass and its retry bitmaps index
  // counted (unchunked) only
  size_t cells = 0, count_bytes = 0;  // (bucket, workgroup) counts and their offsets
};
// n selected-from rows, record bytes rb; staged / sblock: the scatter kernel (part_staged_ok,
// pscatter_block_for).
inline PartGeometry part_geometry(int64_t n, int num_cus, int log2p, bool staged, int sblock, size_t rb, const AggKnobs& K) {
  PartGeometry G;
  G.np = (int64_t)1 << log2p;
  // count / scatter workgroups per CU (QE_PART_WG_PER_CU overrides; see pscatter_block)
  // (one 1024-thread staged workgroup fits a CU)
  G.g = std::min<int64_t>((int64_t)num_cus * (sblock == 1024 ? 1 : K.part_wg_per_cu), ceil_div(n, 256));
  // Chunked scatter (staged buckets): no count pass and no read-back of the record count;
  // workgroups claim PART_CH-record chunks per bucket from a device counter. Record space: every
  // selected row in a full chunk plus one open chunk per (workgroup, bucket) — at most
  // n / PART_CH + g x buckets chunks — so it is taken while the open chunks' slots do not exceed
  // the batch's rows (large batches). QE_PART_CHUNKED (read per call): 0 never, 1 whenever the
  // scatter is staged, unset: by that rule.
  // (forced on a small batch, the scatter runs fewer workgroups so that the open chunks stay
  // within 4x the rows: tests exercise the chunked path at their sizes)
  if (K.part_chunked == 1 && staged && G.g * G.np * PART_CH > 4 * n) G.g = std::max<int64_t>(1, 4 * n / (G.np * PART_CH));
  G.tw = ceil_div(ceil_div(n, G.g), 256) * 256;
  G.g = ceil_div(n, G.tw);
  G.open_slots = G.g * G.np * PART_CH;
  // chunk ids: every claim of a device-wide counter, or each workgroup's own range (part_static)
  G.cmax = std::max<int64_t>(ceil_div(n, PART_CH) + G.g * G.np + 1, G.g * (ceil_div(G.tw, PART_CH) + G.np));
  G.chunked = K.part_chunked != 0 && staged && G.np <= CHUNK_PLAN_MAXB && (K.part_chunked == 1 || G.open_slots <= n) &&
              (uint64_t)G.cmax * PART_CH * rb <= PART_REC_MAX_BYTES;
  if (G.chunked) {
    G.table = chunk_table(G.cmax, G.np);
    G.rec_slots = G.cmax * PART_CH;
    G.rec_bytes = (size_t)G.rec_slots * rb;
    // aggregation slices: at most QE_PAGG_SLICES_PER_CU (default 8) per CU. One 1024-thread
    // workgroup runs per CU either way; more slices balance better, fewer flush less (each slice
    // of a bucket flushes every group it saw with device-scope atomics)
    G.tmax = (int64_t)num_cus * K.pagg_slices_per_cu;
    G.max_slices = G.tmax + G.np;
    G.slice_bytes = (size_t)(2 + 2 * G.max_slices) * 8;
  } else {
    G.cells = (size_t)G.np * (size_t)G.g;
    G.count_bytes = (2 * G.cells + 1) * 8;
  }
  return G;
}

// Counted scatter, once the record count R is read back. Aggregation slices inside bucket
// boundaries: one per bucket, or more (up to 8 per CU, none below ~32K records) when there are few
// buckets; cw is 5/4 of the even share, so a bucket of about average size is one slice, whose
// workgroup then owns its groups outright (plain combines, k_part_slices)
struct CountedSlices {
  int64_t cw = 0, max_slices = 0;
  size_t slice_bytes = 0;
};
inline CountedSlices counted_slices(int64_t R, int64_t np, int num_cus) {
  CountedSlices S;
  const int64_t target = std::max<int64_t>(np, std::min<int64_t>((int64_t)num_cus * 8, R >> 15));
  S.cw = std::max<int64_t>(256, ceil_div(std::max<int64_t>(R, 1) * 5, target * 4));
  S.max_slices = np + ceil_div(std::max<int64_t>(R, 1), S.cw);
  S.slice_bytes = (size_t)(2 + 2 * S.max_slices) * 8;
  return S;
}

// ---- spilling pass (spill_update) ---------------------------------------------------------------
// Sub-buckets of the spilled share of a plan with mp_n key-hash buckets (a power of two, <= 8); 0:
// no spilling pass (QE_MP_SPILL=0, or not that many buckets).
inline int spill_sub_buckets(const AggKnobs& K, int mp_n) {
  const int SB = mp_n - 1;
  return K.mp_spill && mp_n >= 2 && SB <= 8 && !(SB & (SB - 1)) ? SB : 0;
}

struct SpillGeometry {
  int sgrid = 0;     // workgroups of the spilling pass
  int64_t cmax = 0;  // chunk ids
  ChunkTable table;
  int64_t rec_slots = 0;  // cmax * PART_CH
  size_t rec_bytes = 0, slice_bytes = 0;
  int64_t tmax = 0;    // aggregation slices of the spilled share (+ one per sub-bucket)
  uint64_t mp_keep = 0;  // key hashes below it stay in the kept table (2^32 = all)
};
// rows of the batch, bpc / sblock: the spilling kernel's workgroups per CU and threads, SB
// sub-buckets, rb record bytes, kept_slots: slots of the kept (compact or regular) table.
inline SpillGeometry spill_geometry(int64_t rows, int num_cus, int bpc, int sblock, int SB, size_t rb, int64_t kept_slots,
                                    int64_t expected_groups, const AggKnobs& K) {
  SpillGeometry G;
  const int64_t waves = ceil_div(rows, 256);
  G.sgrid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)num_cus * std::max(1, bpc), ceil_div(waves, sblock / 64)));
  // chunks: the full ones plus one open chunk per wave of the grid and sub-bucket
  G.cmax = ceil_div(rows, PART_CH) + (int64_t)G.sgrid * (sblock / 64) * SB + 1;
  G.table = chunk_table(G.cmax, SB);
  G.rec_slots = G.cmax * PART_CH;
  G.rec_bytes = (size_t)G.rec_slots * rb;
  G.tmax = num_cus;
  G.slice_bytes = (size_t)(2 + 2 * (G.tmax + SB)) * 8;
  // kept share: as many groups as one LDS table holds at a 6/8 load, the rest spilled (4096
  // expected groups of the C4 shape: 75 % kept, half the records of an even split; 1B rows, 4096 /
  // 5000 groups: 5/8 7.27 / 8.12 ms, 6/8 6.56 / 7.85, 7/8 6.62 / 10.79). The compact kept table
  // too since round 6's record-major spill (7,000 groups, 1B rows, spilling pass + aggregation
  // pass: 4/8 5.30 + 3.08 ms, 5/8 5.09 + 1.05, 6/8 4.94 + 0.61, 7/8 5.95 + 0.40)
  const double keep = std::min(1.0, (double)(kept_slots * K.spill_load / 8) / (double)std::max<int64_t>(1, expected_groups));
  G.mp_keep = (uint64_t)(keep * 4294967296.0);
  return G;
}

}  // namespace qe
