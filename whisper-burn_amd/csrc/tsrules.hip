// Timestamp-token decoding: Whisper's timestamp rules as a logit filter with per-row state, and the pick under it.
//
// Ids T = [tb, tb + n_ts) are timestamps, N is every other id.  With gen = the tokens generated so far, the allowed set of
// the position being decided is everything not suppressed (suppress[v]; at the first position also suppress_first[v]) minus
//   (a) gen[-1] in T and (len(gen) < 2 or gen[-2] in T): all of T            (timestamps come in pairs)
//   (b) gen[-1] in T and gen[-2] not in T: every id < end-of-text outside T  (a pair is closed before text goes on)
//   (c) with t the last generated timestamp: ids of T below t in case (b), below t + 1 otherwise   (never decreasing)
//   (d) len(gen) == 0: all of N, and ids of T above tb + max_initial_timestamp_index (-1: no limit); with n_ts == 0 the
//       vocabulary has no timestamps and (d) removes nothing: the rules are off, the pick is sample.hip's draw
//   (e) ids of T above tb + max_timestamp_index (-1: none)
//   (f) with ts_lse = logsumexp over the allowed T and mN = max over the allowed N: if ts_lse > mN, all of N.
// The token is the argmax over what is left: of the logit itself at 1 / T = 0, of the key (x - M) / T + g of sample.hip (same
// Philox counters (v >> 2, position, stream, attempt)) otherwise, in the strict total order (key descending, id ascending).
// Recorded with it: x[token] - logsumexp(allowed), the log-probability under the filters (not under x / T).
//
// One pass over the row.  Whether an id is allowed follows from its class (one range test), a handful of block-uniform words
// (the filter of the position: TsFilter) and its suppress byte, so no mask array of the row exists anywhere; each thread keeps
// an online (max, sum exp(x - max)) pair and the best (key, id) for T and for N separately -- one exp per element -- and
// rule (f) is decided from the reduced pairs.  A second pass would read the row (up to 207 KB) again behind a block-wide
// barrier, and this kernel sits on the critical path of every step.
//
// Determinism: the dealing of ids to threads is fixed by the block size (TS_NT threads, TS_PF groups of 4 ids in flight), each
// thread folds its ids in ascending order, the wave reduction is a fixed butterfly and the 16 waves are folded through LDS in
// wave order.  The sums, the decision of rule (f), the token and the log-prob are therefore pure functions of the logits row,
// the row's rule state and the five draw integers: the same in every launch shape and batch, bit-identical from run to run.
//
//   dec_ts_update_kernel   behind the logits tail of a chained timestamp step (decode_step.cpp), in the place and the launch
//                          shape of dec_sample_update_kernel: one block per live row picks the row's token, records it, updates
//                          the row's rule state and prepares the row for the next step.  Plain launch: no block waits for
//                          another block.
//   ts_rows_kernel         the filter + pick alone on caller data (test hook wb_timestamp_rows): the same device function.
#include <hip/hip_runtime.h>

#include "tsrules.h"      // ts_filter, ts_row_pick and their statistics: shared with tsbeam.hip

namespace wb {
namespace {

__global__ __launch_bounds__(TS_NT) void dec_ts_update_kernel(TsChainArgs a) {
  __shared__ TsScratch sc;
  const StepLayout& L = a.lay;
  const TsChainLayout& B = a.tl;
  int* st = a.state;
  int* ctl = a.ctl;
  const int r = blockIdx.x, tid = threadIdx.x;
  // the row's words as they stand at kernel entry: every block reads and writes its own row only; ST_STEP belongs to block 0
  // and ST_N is written at most once per chain, by the block whose row finishes last (as in dec_sample_update_kernel)
  const int n_live = st[ST_N];
  if (r >= n_live || r >= B.S) return;
  const int len_now = st[L.len + r], tok_now = st[L.tok + r], w = st[L.win + r];
  const int fin_now = ctl[B.fin + r], ngen = ctl[B.ngen + r];
  int tok_next = tok_now, fin = fin_now;
  if (!fin_now && ngen < B.max_depth) {          // (block-uniform)
    TsRules R;
    R.tb = ctl[TC_TB]; R.n_ts = ctl[TC_NTS]; R.max_init = ctl[TC_MAX_INIT]; R.max_ts = ctl[TC_MAX_TS]; R.eot = a.eot;
    TsRowState rs;
    rs.n_gen = ngen; rs.last_was = ctl[B.last_was + r]; rs.penult_was = ctl[B.penult_was + r]; rs.last_ts = ctl[B.last_ts + r];
    const float* x = a.logits + (int64_t)r * a.V;
    const TsPick pk = ts_row_pick(x, a.V, ngen == 0 ? a.sup_first : a.sup, ts_filter(R, rs), a.row_stats[2 * r],
                                  __int_as_float(ctl[TC_INVT]), (uint32_t)ctl[TC_SEED_LO], (uint32_t)ctl[TC_SEED_HI],
                                  (uint32_t)ctl[B.stream + r], (uint32_t)ctl[TC_ATTEMPT], (uint32_t)len_now, sc);
    // a NaN logit or a row with no allowed id ends the row on <|endoftext|> and fails the call: never an embedding index
    const bool bad = pk.bad != 0 || (unsigned)pk.id >= (unsigned)a.V;
    tok_next = bad ? a.eot : pk.id;
    fin = tok_next == a.eot ? 1 : 0;
    if (tid == 0) {
      double* sum = reinterpret_cast<double*>(ctl + B.sum);
      if (bad) ctl[TC_ERR] = 1;
      else sum[r] += (double)(x[tok_next] - pk.lse);
      const int is_ts = (!bad && (unsigned)(tok_next - R.tb) < (unsigned)R.n_ts) ? 1 : 0;
      ctl[B.tokens + r * B.max_depth + ngen] = tok_next;
      ctl[B.ngen + r] = ngen + 1;
      ctl[B.penult_was + r] = rs.last_was;
      ctl[B.last_was + r] = is_ts;
      if (is_ts) ctl[B.last_ts + r] = tok_next;
      if (fin) {
        ctl[B.fin + r] = 1;
        // the window's last row: no block streams its cached K/V any more
        if (atomicAdd(&ctl[B.win_fin + w], 1) + 1 == ctl[TC_BEST_OF]) st[L.win_nb + w] = 0;
        if (atomicAdd(&ctl[TC_NDONE], 1) + 1 == ctl[TC_NROWS]) { ctl[TC_ALLDONE] = 1; st[ST_N] = 0; }
      }
    }
  }
  if (len_now >= a.Lmax) return;
  __syncthreads();                               // every thread has read the row's state words (a finished row takes no pick, so
                                                 // no barrier lies behind it): thread 0 may now overwrite them
  // ---- the row's next step: position len_now holds tok_next (a finished row keeps its token and streams nothing) ----
  const int nstep = len_now;                     // = ST_STEP + 1: every row of a chain has the same length
  if (tid == 0) {
    st[L.tok + r] = tok_next;
    st[L.parent + r] = r;
    st[L.len + r] = len_now + 1;
    st[L.dead + r] = fin;
    if (r == 0) st[ST_STEP] = nstep;
  }
  int* tab_new = a.tabs + (size_t)(nstep & 1) * L.S * a.Lmax;
  const int* tab_old = a.tabs + (size_t)((nstep & 1) ^ 1) * L.S * a.Lmax;
  for (int p = tid; p < len_now; p += TS_NT) tab_new[r * a.Lmax + p] = tab_old[r * a.Lmax + p];
  if (tid == 0) tab_new[r * a.Lmax + len_now] = nstep * L.S + r;
  const float4* e = reinterpret_cast<const float4*>(a.E + (int64_t)tok_next * a.d);
  const float4* pp = reinterpret_cast<const float4*>(a.pos + (int64_t)len_now * a.d);
  float4* o = reinterpret_cast<float4*>(a.x + (int64_t)r * a.d);
  for (int c = tid; c < (a.d >> 2); c += TS_NT) {
    const float4 u = e[c], v = pp[c];
    o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}

__global__ __launch_bounds__(TS_NT) void ts_rows_kernel(TsRowsArgs a) {
  __shared__ TsScratch sc;
  const int r = blockIdx.x;
  if (r >= a.R) return;
  const float* x = a.logits + (int64_t)r * a.ld;
  const int tb = a.rules.tb, n_ts = a.rules.n_ts;
  TsRowState rs;
  rs.n_gen = a.n_gen[r];
  rs.last_was = (unsigned)(a.prev1[r] - tb) < (unsigned)n_ts ? 1 : 0;
  rs.penult_was = (unsigned)(a.prev2[r] - tb) < (unsigned)n_ts ? 1 : 0;
  rs.last_ts = a.last_ts[r];
  const TsPick pk = ts_row_pick(x, a.V, rs.n_gen == 0 ? a.sup_first : a.sup, ts_filter(a.rules, rs), a.row_max[r], a.inv_t,
                                a.seed_lo, a.seed_hi, (uint32_t)a.stream[r], a.attempt, (uint32_t)a.position[r], sc);
  if (threadIdx.x == 0) {
    const bool bad = pk.bad != 0 || (unsigned)pk.id >= (unsigned)a.V;
    const int tok = bad ? a.rules.eot : pk.id;
    if (bad) *a.out_err = 1;
    a.out_token[r] = tok;
    a.out_logprob[r] = bad ? 0.f : x[tok] - pk.lse;
    a.out_forced[r] = bad ? 0 : pk.forced;
    a.out_stats[2 * r] = pk.ts_lse;
    a.out_stats[2 * r + 1] = pk.mN;
  }
}

}  // namespace

void launch_dec_ts_update(hipStream_t st, const TsChainArgs& a, int n_rows) {
  WB_KLAUNCH(dec_ts_update_kernel, dim3(n_rows), dim3(TS_NT), 0, st, a);
}

void launch_ts_rows(hipStream_t st, const TsRowsArgs& a) {
  WB_KLAUNCH(ts_rows_kernel, dim3(a.R), dim3(TS_NT), 0, st, a);
}

}  // namespace wb
