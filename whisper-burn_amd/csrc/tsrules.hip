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

#include "decode.h"
#include "philox.h"
#include "wave_ops.h"

namespace wb {
namespace {

constexpr int TS_NT = 1024, TS_NW = TS_NT / 64;
constexpr int TS_PF = 4;             // groups (4 ids each) per thread whose loads are requested together: 16 logits in flight

// the filter of one position, block-uniform: T ids are allowed inside [t_lo, t_hi] (empty: t_lo > t_hi)
struct TsFilter { int tb, n_ts, t_lo, t_hi, rm_n, rm_text, eot; };

__device__ __forceinline__ TsFilter ts_filter(const TsRules& R, const TsRowState& s) {
  const bool first = s.n_gen == 0;
  const bool last_was = s.n_gen >= 1 && s.last_was != 0;
  const bool case_a = last_was && (s.n_gen < 2 || s.penult_was != 0);
  const bool case_b = last_was && !case_a;
  int lo = R.tb, hi = R.tb + R.n_ts - 1;
  if (s.last_ts >= 0) lo = max(lo, case_b ? s.last_ts : s.last_ts + 1);                           // (c)
  if (R.max_ts >= 0 && R.max_ts < R.n_ts - 1) hi = R.tb + R.max_ts;                               // (e)
  if (first && R.max_init >= 0 && R.max_init < R.n_ts - 1) hi = min(hi, R.tb + R.max_init);       // (d)
  if (case_a) { lo = 1; hi = 0; }                                                                 // (a)
  TsFilter f;
  f.tb = R.tb; f.n_ts = R.n_ts; f.t_lo = lo; f.t_hi = hi; f.rm_n = (first && R.n_ts > 0) ? 1 : 0; f.rm_text = case_b ? 1 : 0; f.eot = R.eot;
  return f;
}

// online (max, sum exp(x - max)), score.hip's scheme: one exp per element; x is finite or +inf here
__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
  if (x > m) { s = s * expf(m - x) + 1.f; m = x; }          // (m = -inf: s = 0 * 0 + 1)
  else s += expf(x - m);
}
__device__ __forceinline__ void lse_fold(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) return;                               // both empty
  s = s * expf(m - M) + os * expf(om - M);
  m = M;
}
// (max, sum) over the 64 lanes, valid in lane 63 and broadcast from there (the butterfly of wave_sum)
__device__ __forceinline__ void wave_lse(float& m, float& s) {
#define WB_STEP(CTRL, MASK)                                                 \
  {                                                                         \
    const float om = dpp_f<CTRL, MASK>(-INFINITY, m);                       \
    const float os = dpp_f<CTRL, MASK>(0.f, s);                             \
    lse_fold(m, s, om, os);                                                 \
  }
  WB_STEP(DPP_QUAD_XOR1, 0xF)
  WB_STEP(DPP_QUAD_XOR2, 0xF)
  WB_STEP(DPP_ROW_HALF_MIRROR, 0xF)
  WB_STEP(DPP_ROW_MIRROR, 0xF)
  WB_STEP(DPP_ROW_BCAST15, 0xA)
  WB_STEP(DPP_ROW_BCAST31, 0xC)
#undef WB_STEP
  m = readlane63(m);
  s = readlane63(s);
}

struct TsScratch {
  float mT[TS_NW], sT[TS_NW], mN[TS_NW], sN[TS_NW], kT[TS_NW], kN[TS_NW];
  int iT[TS_NW], iN[TS_NW], bad[TS_NW];
};

struct TsPick { int id; int bad; int forced; float ts_lse, mN, lse; };

// The pick of one row by one block of TS_NT threads (every thread of the block calls it; two barriers inside).
// x [V]: the row's logits; sup: the suppress bytes of this position, 4 ids per word, or null; M: the row maximum over all ids
// (only the shift of the keys: any value gives the same order up to rounding, this one gives sample.hip's keys).  Returns,
// in every thread, the token (0x7fffffff: no id is allowed), `bad` != 0 when a logit of the row was NaN or the sums are not
// finite, the decision of rule (f) and the statistics it was taken from.
__device__ __forceinline__ TsPick ts_row_pick(const float* __restrict__ x, int V, const uint32_t* __restrict__ sup, const TsFilter f,
                                              float M, float inv_t, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t attempt,
                                              uint32_t position, TsScratch& sc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = (V + 3) >> 2;
  const bool draw = inv_t != 0.f;
  float mT = -INFINITY, sT = 0.f, mN = -INFINITY, sN = 0.f, kT = -INFINITY, kN = -INFINITY;
  int iT = 0x7fffffff, iN = 0x7fffffff, bad = 0;
  for (int g0 = tid; g0 < G; g0 += TS_NT * TS_PF) {
    float xb[TS_PF][4];
    uint32_t sb[TS_PF];
#pragma unroll
    for (int u = 0; u < TS_PF; u++) {
      const int g = g0 + TS_NT * u;
      sb[u] = sup ? sup[g < G ? g : 0] : 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int c = 4 * g + q, cc = c < V ? c : 0;                      // (past the row: re-read id 0, discarded below)
        xb[u][q] = x[cc];
      }
    }
#pragma unroll
    for (int u = 0; u < TS_PF; u++) {
      const int g = g0 + TS_NT * u;
      if (4 * g < V) {
        U4 r;
        if (draw) r = philox4x32_10((uint32_t)g, position, stream, attempt, k0, k1);
        else { r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u; }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = 4 * g + q;
          if (c < V) {
            const float xv = xb[u][q];
            if (xv != xv) bad = 1;
            const bool is_t = (unsigned)(c - f.tb) < (unsigned)f.n_ts;
            const bool supd = ((sb[u] >> (8 * q)) & 0xffu) != 0u;
            const bool ok = !supd && (is_t ? (c >= f.t_lo && c <= f.t_hi) : (!f.rm_n && !(f.rm_text && c < f.eot)));
            if (ok && xv > -INFINITY) {                                     // (false for NaN)
              const float key = draw ? fmaf(xv - M, inv_t, gumbel_of(r.w[q])) : xv;
              if (key != key) bad = 1;
              if (is_t) {
                lse_push(mT, sT, xv);
                if (better(key, c, kT, iT)) { kT = key; iT = c; }
              } else {
                lse_push(mN, sN, xv);
                if (better(key, c, kN, iN)) { kN = key; iN = c; }
              }
            }
          }
        }
      }
    }
  }
  wave_lse(mT, sT);
  wave_lse(mN, sN);
  wave_argmax(kT, iT);
  wave_argmax(kN, iN);
  const int wbad = __ballot(bad) != 0ull ? 1 : 0;
  if (lane == 0) {
    sc.mT[wave] = mT; sc.sT[wave] = sT; sc.mN[wave] = mN; sc.sN[wave] = sN;
    sc.kT[wave] = kT; sc.iT[wave] = iT; sc.kN[wave] = kN; sc.iN[wave] = iN; sc.bad[wave] = wbad;
  }
  __syncthreads();
  mT = sc.mT[0]; sT = sc.sT[0]; mN = sc.mN[0]; sN = sc.sN[0];
  kT = sc.kT[0]; iT = sc.iT[0]; kN = sc.kN[0]; iN = sc.iN[0]; bad = sc.bad[0];
  for (int j = 1; j < TS_NW; j++) {                                         // the waves in wave order
    lse_fold(mT, sT, sc.mT[j], sc.sT[j]);
    lse_fold(mN, sN, sc.mN[j], sc.sN[j]);
    if (better(sc.kT[j], sc.iT[j], kT, iT)) { kT = sc.kT[j]; iT = sc.iT[j]; }
    if (better(sc.kN[j], sc.iN[j], kN, iN)) { kN = sc.kN[j]; iN = sc.iN[j]; }
    bad |= sc.bad[j];
  }
  __syncthreads();                       // (the scratch words may be reused by the caller)
  TsPick o;
  o.ts_lse = mT + logf(sT);              // (no allowed timestamp: -inf + -inf)
  o.mN = mN;
  const float n_lse = mN + logf(sN);
  o.forced = o.ts_lse > mN ? 1 : 0;                                         // (f)
  const float hi = fmaxf(o.ts_lse, n_lse), lo = fminf(o.ts_lse, n_lse);
  o.lse = o.forced ? o.ts_lse : (hi == -INFINITY ? hi : hi + log1pf(expf(lo - hi)));
  o.id = (o.forced || better(kT, iT, kN, iN)) ? iT : iN;
  o.bad = (bad != 0 || !(fabsf(o.lse) < INFINITY)) ? 1 : 0;                 // (an allowed +inf logit has no log-prob; NaN compares false)
  return o;
}

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
