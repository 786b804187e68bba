// The three fused GROUP BY plans the host programs build without a GPU (gen_sources.cpp emits
// their kernel sources, agg_paths.cpp plans their paths): c4, the nullable fp64 MAX plan f64max and
// the exact fp64 SUM / AVG plan det. Key in slot 0; aggregates given as (fn, acc, program).
#pragma once

#include <stdio.h>
#include <string.h>

#include "qe_internal.hpp"

struct AggIn {
  int fn, acc;
  const qe_agg_program* prog;  // null: COUNT(*)
};

inline qe_pred_term term(int col, int op, int64_t lit) {
  qe_pred_term t;
  memset(&t, 0, sizeof t);
  t.col = col;
  t.op = op;
  t.rhs_col = -1;
  t.lit.type = QE_TYPE_INT64;
  t.lit.bits = lit;
  return t;
}

// The Plan of one such query, as compile_plan builds it (token programs in their general form).
inline int make_agg_plan(const char* name, const qe_column* cols, int ncols, const qe_pred_term* terms, int nterms,
                         const AggIn* aggs, int naggs, qe::Plan* out) {
  using namespace qe;
  Plan& P = *out;
  bool col_f64[QE_MAX_COLS];
  if (compile_inputs(cols, ncols, -1, nterms, terms, &P, col_f64) != QE_OK) {
    fprintf(stderr, "%s: compile_inputs: %s\n", name, qe_last_error());
    return 1;
  }
  P.key_mode = 1;
  P.nkeys = 1;
  P.key_col[0] = 0;
  P.key_f64 = 0;
  P.naggs = naggs;
  for (int j = 0; j < naggs; ++j) {
    memset(&P.aggs[j], 0, sizeof P.aggs[j]);
    bool is_f = false, nullable = false;
    if (aggs[j].prog && compile_program(cols, ncols, col_f64, *aggs[j].prog, j, &P.aggs[j], &is_f, &nullable) != QE_OK) {
      fprintf(stderr, "%s: compile_program: %s\n", name, qe_last_error());
      return 1;
    }
    P.aggs[j].fn = aggs[j].fn;
    P.aggs[j].acc = aggs[j].acc;
    P.aggs[j].track_nn = nullable ? 1 : 0;
    P.aggs[j].pkind = aggs[j].prog ? 2 : 0;  // token program (compile_plan's general form)
  }
  // the same input summed twice (SUM and AVG of one column): one shared LDS accumulator, as
  // compile_plan marks it
  for (int j = 1; j < naggs; ++j)
    if (aggs[j].prog && aggs[j].prog == aggs[0].prog && aggs[j].acc == aggs[0].acc) P.aggs[j].share = 1;
  return 0;
}

// fn(name, cols, ncols, terms, nterms, aggs, naggs, log2) for c4, f64max and det; ORs the results.
template <typename F>
inline int for_each_agg_plan(F&& fn) {
  using namespace qe;
  static int64_t dummy[64];
  static uint8_t vdummy[64];
  static double fdummy[64];
  qe_column cols[3];
  memset(cols, 0, sizeof cols);
  for (int c = 0; c < 3; ++c) {
    cols[c].type = QE_TYPE_INT64;
    cols[c].length = 1000;
    cols[c].values = dummy;
  }
  // C4: SELECT k, SUM(a+b), COUNT(*), MIN(a), MAX(b) WHERE a > 2^19 GROUP BY k (slots k, a, b)
  qe_pred_term t4 = term(1, QE_OP_GT, 1 << 19);
  qe_agg_program ab, pa, pb;
  memset(&ab, 0, sizeof ab);
  ab.ntokens = 3;
  ab.tokens[0].op = QE_TOK_COL;
  ab.tokens[0].arg = 1;
  ab.tokens[1].op = QE_TOK_COL;
  ab.tokens[1].arg = 2;
  ab.tokens[2].op = QE_TOK_ADD;
  memset(&pa, 0, sizeof pa);
  pa.ntokens = 1;
  pa.tokens[0].op = QE_TOK_COL;
  pa.tokens[0].arg = 1;
  pb = pa;
  pb.tokens[0].arg = 2;
  const AggIn c4[4] = {{QE_AGG_SUM, ACC_SUM_I, &ab}, {QE_AGG_COUNT_STAR, ACC_NONE, nullptr},
                       {QE_AGG_MIN, ACC_MIN_I, &pa}, {QE_AGG_MAX, ACC_MAX_I, &pb}};
  int rc = fn("c4", cols, 3, &t4, 1, c4, 4, 12);
  // nullable key and an fp64 MAX (records carry flags and the global row index)
  cols[0].validity = vdummy;
  cols[2].type = QE_TYPE_FLOAT64;
  cols[2].values = fdummy;
  cols[2].validity = vdummy;
  const AggIn fx[2] = {{QE_AGG_MAX, ACC_MAX_F, &pb}, {QE_AGG_COUNT_STAR, ACC_NONE, nullptr}};
  rc |= fn("f64max", cols, 3, &t4, 1, fx, 2, 11);
  // deterministic state: fp64 SUM and AVG in exact fixed point (ACC_SUM_X)
  const AggIn dx[3] = {{QE_AGG_SUM, ACC_SUM_X, &pb}, {QE_AGG_AVG, ACC_SUM_X, &pb}, {QE_AGG_COUNT_STAR, ACC_NONE, nullptr}};
  rc |= fn("det", cols, 3, &t4, 1, dx, 3, 10);
  return rc;
}
