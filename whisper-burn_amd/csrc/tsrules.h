// The timestamp rules as device functions, shared by tsrules.hip (greedy / sampled rows) and tsbeam.hip (beam search under
// the rules): the filter of one position from the row's rule state, the online (max, sum) statistics and the one-pass pick of
// one row by one block.  See the head of tsrules.hip for the rules and the determinism argument.
#pragma once
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

// whether id c (suppress byte `supd`) passes rules (a) - (e) and the static masks
__device__ __forceinline__ bool ts_allowed(const TsFilter& f, int c, bool supd, bool& is_t) {
  is_t = (unsigned)(c - f.tb) < (unsigned)f.n_ts;
  return !supd && (is_t ? (c >= f.t_lo && c <= f.t_hi) : (!f.rm_n && !(f.rm_text && c < f.eot)));
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

}  // namespace
}  // namespace wb
