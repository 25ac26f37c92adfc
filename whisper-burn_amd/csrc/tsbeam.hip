// Beam search under the timestamp rules: Whisper's BeamSearchDecoder with the per-beam rule state on the device.
//
// Per window, with B = beam_size and C = max_candidates (both in the control block):
//   * one live beam holds the prompt with score 0 (Whisper's B identical copies collapse to it);
//   * a live beam's candidates are its min(B + 1, |allowed|) best allowed ids by (logit descending, id ascending), allowed =
//     rules (a) - (f) of tsrules.hip over the beam's OWN rule state, each with lp = x - logsumexp(allowed) in f32 and the
//     score = the beam's score + (double)lp;
//   * the window's candidates are ranked by (score descending, beam index ascending, rank within the beam ascending) and
//     walked in that order: an end-of-text candidate is newly finished, any other becomes a live beam of the next step, and
//     the walk stops behind the B-th live beam (end-of-text candidates ranked behind that point are dropped);
//   * the newly finished enter the store in walk order while it holds fewer than C entries; the window ends when the store
//     holds C entries or no live beam is left;
//   * a child's rule state is its parent's, updated by the child's token as dec_ts_update_kernel updates a row's.
//
//   dec_tsbeam_rows_kernel    one block per live row behind the logits tail (the place of dec_ts_update_kernel).  Pass 1 is
//                             ts_row_pick itself (tsrules.h): the class statistics, rule (f) and logsumexp(allowed) -- the same
//                             bits as the greedy path.  Rule (f) is known only then, so the B + 1 best ids come from a SECOND
//                             pass over the row (<= 207 KB, L2-resident behind pass 1): a scan for the waves' best ids gives a
//                             floor (the k-th best of the 16), then each thread keeps the TOPK_MAX best of its ids above
//                             the floor in registers (compare-and-swap chain with constant indices: no scratch), then k
//                             rounds of a block-wide argmax pop the winners in order.  The alternative -- a top-K list per
//                             class in pass 1, merged after the decision -- doubles the list registers and the insertion
//                             work on every element of the pass that the greedy path shares.
//   dec_tsbeam_update_kernel  one block, one wave per window (dec_beam_update_kernel's structure): every lane owns one
//                             candidate and computes its rank by counting, not by serial insertion.  Appends (token, parent
//                             node) to the node tree, records the trace (score and parent of every live beam per depth),
//                             writes the next step's state block, parent slots, position tables and embedding rows, counts
//                             ended windows and blanks ST_N when all have ended.
// Both are plain launches: no block waits for another block.  Determinism: pass 1 as tsrules.hip; the second pass deals ids
// to threads by the block size alone and the order (logit, id) is total, so ids, log-probs and ranks are pure functions of
// the logits rows and the beams' states.
#include "tsrules.h"

namespace wb {
namespace {

struct TbScratch { float v[TS_NW]; int i[TS_NW]; };

// BODY for every id c (logit xv) of the row that is allowed under the final filter (rules (a) - (e), the static masks, `forced`:
// timestamps only; finite logits), in ascending id order per thread; TS_PF groups of 4 ids per thread are requested together,
// as in ts_row_pick (one group per trip measured 13 dependent round trips per scan)
#define TSBEAM_SCAN(...)                                                                                                \
  for (int g0 = tid; g0 < G; g0 += TS_NT * TS_PF) {                                                                     \
    float xb[TS_PF][4];                                                                                                 \
    uint32_t sb[TS_PF];                                                                                                 \
    _Pragma("unroll") for (int u = 0; u < TS_PF; u++) {                                                                 \
      const int g = g0 + TS_NT * u;                                                                                     \
      sb[u] = sup ? sup[g < G ? g : 0] : 0u;                                                                            \
      _Pragma("unroll") for (int q = 0; q < 4; q++) { const int cq = 4 * g + q; xb[u][q] = x[cq < V ? cq : 0]; }        \
    }                                                                                                                   \
    _Pragma("unroll") for (int u = 0; u < TS_PF; u++) {                                                                 \
      const int g = g0 + TS_NT * u;                                                                                     \
      _Pragma("unroll") for (int q = 0; q < 4; q++) {                                                                   \
        const int c = 4 * g + q;                                                                                        \
        const float xv = xb[u][q];                                                                                      \
        bool is_t;                                                                                                      \
        if (c < V && ts_allowed(f, c, ((sb[u] >> (8 * q)) & 0xffu) != 0u, is_t) && (!forced || is_t) && xv > -INFINITY) { __VA_ARGS__ } \
      }                                                                                                                 \
    }                                                                                                                   \
  }

// The k best ids of the row under the final filter (rules (a) - (e) + the static masks; `forced`: timestamps only), in
// (logit descending, id ascending) order, by the whole block.  Thread 0 writes out_id / out_lp [count]; returns the count in
// every thread.  Barriers inside: every thread of the block calls it with block-uniform arguments.
__device__ __forceinline__ int tsbeam_row_topk(const float* __restrict__ x, int V, const uint32_t* __restrict__ sup, const TsFilter f,
                                               int forced, float lse, int k, TbScratch& tb, int32_t* __restrict__ out_id,
                                               float* __restrict__ out_lp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = (V + 3) >> 2;
  // ---- a floor for the lists: the k-th best of the 16 waves' best ids.  k ids are at least that good, so an id below it is
  // not among the k best of the row; a wave on a 64-lane SIMD16 pays for the insertion chain below whenever ANY of its lanes
  // inserts, which without a floor is at nearly every id (measured: 57 us of the kernel's 111 at 15 rows of 51864 ids)
  float fv = -INFINITY;
  int fi = 0x7fffffff;
  TSBEAM_SCAN(if (better(xv, c, fv, fi)) { fv = xv; fi = c; })
  wave_argmax(fv, fi);
  if (lane == 0) { tb.v[wave] = fv; tb.i[wave] = fi; }
  __syncthreads();
  {  // lane a < 16 of every wave ranks wave a's best among the 16 (every thread doing all 256 comparisons measured ~25 us)
    const int a = lane & (TS_NW - 1);
    const float av = tb.v[a];
    const int ai = tb.i[a];
    int n_better = 0;
    for (int b = 0; b < TS_NW; b++) n_better += better(tb.v[b], tb.i[b], av, ai) ? 1 : 0;
    const unsigned long long hit = __ballot(lane < TS_NW && n_better == k - 1);
    fv = -INFINITY; fi = 0x7fffffff;                // (fewer than k waves hold an allowed id: no floor)
    if (hit != 0ull) {                              // (at most one lane: the order is total; empty waves tie, and give no floor)
      const int src = __ffsll((long long)hit) - 1;
      fv = __shfl(av, src); fi = __shfl(ai, src);
    }
  }
  __syncthreads();                                  // (tb is reused by the rounds below)
  float lv[TOPK_MAX];
  int li[TOPK_MAX];
#pragma unroll
  for (int j = 0; j < TOPK_MAX; j++) { lv[j] = -INFINITY; li[j] = 0x7fffffff; }
  TSBEAM_SCAN(if (!better(fv, fi, xv, c) && better(xv, c, lv[TOPK_MAX - 1], li[TOPK_MAX - 1])) {
    float nv = xv;
    int ni = c;
    _Pragma("unroll") for (int j = 0; j < TOPK_MAX; j++)
      if (better(nv, ni, lv[j], li[j])) { const float tv = lv[j]; const int ti = li[j]; lv[j] = nv; li[j] = ni; nv = tv; ni = ti; }
  })
  int count = 0;
  for (int round = 0; round < k; round++) {         // (k and every exit below are block-uniform)
    float v = lv[0];
    int i = li[0];
    wave_argmax(v, i);
    if (lane == 0) { tb.v[wave] = v; tb.i[wave] = i; }
    __syncthreads();
    float bv = lane < TS_NW ? tb.v[lane] : -INFINITY;       // the 16 waves' heads: one per lane, the butterfly again
    int bi = lane < TS_NW ? tb.i[lane] : 0x7fffffff;
    wave_argmax(bv, bi);
    __syncthreads();
    if (bi == 0x7fffffff) break;                    // fewer than k allowed ids
    if (tid == 0) { out_id[round] = bi; out_lp[round] = bv - lse; }
    if (li[0] == bi) {                              // the owner pops its head (ids are unique over the block)
#pragma unroll
      for (int j = 0; j < TOPK_MAX - 1; j++) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
      lv[TOPK_MAX - 1] = -INFINITY; li[TOPK_MAX - 1] = 0x7fffffff;
    }
    count++;
  }
  return count;
}

// One row: statistics + rule (f) (ts_row_pick), then its k best allowed ids.  A NaN logit, an allowed +inf logit or a row
// without an allowed id gives the single candidate end-of-text with log-prob 0 and *err = 1.
__device__ __forceinline__ void tsbeam_row(const float* __restrict__ x, int V, const uint32_t* __restrict__ sup, const TsFilter f, int k,
                                           int eot, TsScratch& sc, TbScratch& tb, int32_t* __restrict__ out_id,
                                           float* __restrict__ out_lp, int* __restrict__ out_count, int* __restrict__ out_forced,
                                           float* __restrict__ out_ts_lse, float* __restrict__ out_mN, int* __restrict__ err) {
  const TsPick pk = ts_row_pick(x, V, sup, f, 0.f, 0.f, 0u, 0u, 0u, 0u, 0u, sc);
  int count = 0;
  if (!pk.bad) count = tsbeam_row_topk(x, V, sup, f, pk.forced, pk.lse, k, tb, out_id, out_lp);
  if (threadIdx.x == 0) {
    const bool bad = pk.bad != 0 || count == 0;
    if (bad) { *err = 1; out_id[0] = eot; out_lp[0] = 0.f; count = 1; }
    *out_count = count;
    *out_forced = bad ? 0 : pk.forced;
    *out_ts_lse = pk.ts_lse;
    *out_mN = pk.mN;
  }
}

__global__ __launch_bounds__(TS_NT) void dec_tsbeam_rows_kernel(TsBeamRowsArgs a) {
  __shared__ TsScratch sc;
  __shared__ TbScratch tb;
  const TsBeamLayout& B = a.bl;
  int* ctl = a.ctl;
  const int r = blockIdx.x;
  if (r >= a.state[ST_N] || r >= B.S) return;
  const int w = a.state[a.lay.win + r], j = ctl[B.row_beam + r];
  const int depth = ctl[TB_DEPTH], k = min(ctl[TB_B] + 1, TOPK_MAX);
  TsRules R;
  R.tb = ctl[TB_TB]; R.n_ts = ctl[TB_NTS]; R.max_init = ctl[TB_MAX_INIT]; R.max_ts = ctl[TB_MAX_TS]; R.eot = a.eot;
  TsRowState rs;
  const int o = w * MAX_BEAMS + j;
  rs.n_gen = depth; rs.last_was = ctl[B.last_was + o]; rs.penult_was = ctl[B.penult_was + o]; rs.last_ts = ctl[B.last_ts + o];
  int* ro = a.row_out + r * TBR_STRIDE;
  tsbeam_row(a.logits + (int64_t)r * a.V, a.V, depth == 0 ? a.sup_first : a.sup, ts_filter(R, rs), k, a.eot, sc, tb,
             a.topk_id + r * TOPK_MAX, a.topk_lp + r * TOPK_MAX, ro + TBR_COUNT, ro + TBR_FORCED,
             reinterpret_cast<float*>(ro + TBR_TS_LSE), reinterpret_cast<float*>(ro + TBR_MN), ctl + TB_ERR);
}

__global__ __launch_bounds__(TS_NT) void tsbeam_rows_hook_kernel(TsBeamRowsHookArgs a) {
  __shared__ TsScratch sc;
  __shared__ TbScratch tb;
  const int r = blockIdx.x;
  if (r >= a.R) return;
  const int tbeg = a.rules.tb, n_ts = a.rules.n_ts;
  TsRowState rs;
  rs.n_gen = a.n_gen[r];
  rs.last_was = (unsigned)(a.prev1[r] - tbeg) < (unsigned)n_ts ? 1 : 0;
  rs.penult_was = (unsigned)(a.prev2[r] - tbeg) < (unsigned)n_ts ? 1 : 0;
  rs.last_ts = a.last_ts[r];
  tsbeam_row(a.logits + (int64_t)r * a.ld, a.V, rs.n_gen == 0 ? a.sup_first : a.sup, ts_filter(a.rules, rs), a.k, a.rules.eot, sc, tb,
             a.out_id + (int64_t)r * a.k, a.out_lp + (int64_t)r * a.k, a.out_count + r, a.out_forced + r, a.out_stats + 2 * r,
             a.out_stats + 2 * r + 1, a.out_err);
}

__global__ __launch_bounds__(1024) void dec_tsbeam_update_kernel(TsBeamUpdateArgs a) {
  constexpr int NW = 16, MB = MAX_BEAMS;            // waves per block = windows per pass
  __shared__ int w_slot[NW][MB], w_node[NW][MB], w_lw[NW][MB], w_lts[NW][MB];
  __shared__ double w_sc[NW][MB];
  __shared__ int c_tok[NW][64], c_rank[NW][64];
  __shared__ double c_sc[NW][64];
  __shared__ int o_tok[NW][MB], o_par[NW][MB];
  __shared__ double o_sc[NW][MB];
  __shared__ int g_tok[64][MB], g_prev[64][MB];     // the next step's rows, kept for every window of the batch (<= 64)
  __shared__ int n_live_w[64], base_w[64], ended_w[64];
  __shared__ int s_tok[64 * MB], s_par[64 * MB];
  __shared__ int n_total;
  const TsBeamLayout& B = a.bl;
  const StepLayout& L = a.lay;
  int* ctl = a.ctl;
  if (ctl[TB_ALLDONE]) return;                      // (block-uniform) a step enqueued behind the end of the search
  double* scv = reinterpret_cast<double*>(ctl + B.score);
  double* fin_sc = reinterpret_cast<double*>(ctl + B.fin_score);
  double* tr_sc = reinterpret_cast<double*>(ctl + B.tr_score);
  int2* nodes = reinterpret_cast<int2*>(ctl + B.nodes);
  const int W = B.W, nB = ctl[TB_B], nC = ctl[TB_C], tbeg = ctl[TB_TB], n_ts = ctl[TB_NTS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int depth = ctl[TB_DEPTH];                  // decode steps completed before this call's step
  for (int w0 = 0; w0 < W; w0 += NW) {              // (block-uniform trip count: every wave meets every barrier)
    const int w = w0 + wv;
    const bool act = w < W;
    const int nb = act ? ctl[B.nb + w] : 0;
    const int was_ended = act ? ctl[B.ended + w] : 1;
    const int nfin = act ? ctl[B.nfin + w] : 0;
    const bool run = act && !was_ended && nb > 0;
    if (lane < MB) {
      const bool on = run && lane < nb;
      const int o = w * MB + lane;
      w_slot[wv][lane] = on ? ctl[B.slot + o] : -1; w_node[wv][lane] = on ? ctl[B.node + o] : -1;
      w_lw[wv][lane] = on ? ctl[B.last_was + o] : 0; w_lts[wv][lane] = on ? ctl[B.last_ts + o] : -1;
      w_sc[wv][lane] = on ? scv[o] : 0.0;
    }
    __syncthreads();
    // ---- candidates: lane = (beam j, rank i within the beam): insertion order of Whisper's candidate dictionary ----
    const int j = lane / TOPK_MAX, i = lane - j * TOPK_MAX;
    int tok = -1; double sc = 0.0; bool cand = false;
    if (run && j < nb) {
      const int slot = w_slot[wv][j];
      const int cnt = min(a.row_out[slot * TBR_STRIDE + TBR_COUNT], nB + 1);
      if (i < cnt) {
        tok = a.topk_id[slot * TOPK_MAX + i];
        sc = w_sc[wv][j] + (double)a.topk_lp[slot * TOPK_MAX + i];
        // never an embedding index: the host fails the call
        if ((unsigned)tok >= (unsigned)a.V) { ctl[TB_ERR] = 1; tok = a.eot; }
        if (!(sc == sc)) { ctl[TB_ERR] = 1; tok = a.eot; sc = -INFINITY; }
        cand = true;
      }
    }
    c_tok[wv][lane] = tok; c_sc[wv][lane] = sc;
    __syncthreads();
    const int n_lanes = run ? nb * TOPK_MAX : 0;
    int rank = 0x7fffffff;
    if (cand) {
      rank = 0;
      for (int c2 = 0; c2 < n_lanes; c2++) {
        const double s2 = c_sc[wv][c2];
        if (c_tok[wv][c2] >= 0 && (s2 > sc || (s2 == sc && c2 < lane))) rank++;
      }
    }
    c_rank[wv][lane] = rank;
    __syncthreads();
    // ---- the walk: live beams in front of this candidate, finished ones in front of it ----
    int lb = 0, fb = 0;
    if (cand)
      for (int c2 = 0; c2 < n_lanes; c2++)
        if (c_tok[wv][c2] >= 0 && c_rank[wv][c2] < rank) { if (c_tok[wv][c2] == a.eot) fb++; else lb++; }
    const bool is_eot = tok == a.eot;
    const bool to_live = cand && !is_eot && lb < nB;
    const bool to_fin = cand && is_eot && lb < nB;   // (an end-of-text behind the B-th live beam is dropped)
    const int n_next = __popcll(__ballot(to_live)), n_newfin = __popcll(__ballot(to_fin));
    if (to_live) {
      const int pool = (depth * W + w) * MB + lb;
      nodes[pool] = make_int2(tok, w_node[wv][j]);
      tr_sc[pool] = sc;
      o_tok[wv][lb] = tok; o_par[wv][lb] = j; o_sc[wv][lb] = sc;
    }
    if (to_fin && nfin + fb < nC) {                  // the store: walk order, at most C entries
      ctl[B.fin_node + w * BEAM_KB + nfin + fb] = w_node[wv][j];
      fin_sc[w * BEAM_KB + nfin + fb] = sc;
    }
    const int nfin_new = min(nC, nfin + n_newfin);
    __syncthreads();
    // ---- the next generation: a child's rule state is its parent's, updated by the child's token ----
    if (run && lane < n_next) {
      const int tk = o_tok[wv][lane], pj = o_par[wv][lane];
      const int is_ts = (unsigned)(tk - tbeg) < (unsigned)n_ts ? 1 : 0;
      const int o = w * MB + lane;
      ctl[B.node + o] = (depth * W + w) * MB + lane;
      scv[o] = o_sc[wv][lane];
      ctl[B.penult_was + o] = w_lw[wv][pj];
      ctl[B.last_was + o] = is_ts;
      ctl[B.last_ts + o] = is_ts ? tk : w_lts[wv][pj];
      g_tok[w][lane] = tk; g_prev[w][lane] = w_slot[wv][pj];
    }
    if (act && lane == 0) {
      const int now_ended = was_ended || (run && (nfin_new >= nC || n_next == 0)) ? 1 : 0;
      if (run) {
        ctl[B.nb + w] = n_next; ctl[B.nfin + w] = nfin_new;
        ctl[B.tr_n + depth * W + w] = n_next; ctl[B.tr_fin + depth * W + w] = n_newfin;
        if (now_ended) ctl[B.ended + w] = 1;
      }
      ended_w[w] = (now_ended || nb == 0) ? 1 : 0;
      n_live_w[w] = (now_ended || !run) ? 0 : n_next;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int acc = 0, n_end = 0;
    for (int q = 0; q < W; q++) { base_w[q] = acc; acc += n_live_w[q]; n_end += ended_w[q]; }
    if (depth + 1 >= B.max_depth) acc = 0;          // the step that just ran was the last one allowed
    ctl[TB_DEPTH] = depth + 1;
    ctl[TB_NENDED] = n_end;
    ctl[TB_NLIVE] = acc;
    if (acc == 0) ctl[TB_ALLDONE] = 1;
    n_total = acc;
  }
  __syncthreads();
  const int n_all = n_total;
  // ---- the next step's state block (ST_N = 0 when every window has ended: steps already enqueued exit at once) ----
  const int step_next = a.step_pos + depth + 1;
  int* so = a.state;
  for (int e = tid; e < L.total; e += 1024) so[e] = e == ST_N ? n_all : (e == ST_STEP ? step_next : 0);
  __syncthreads();
  if (n_all > 0) {
    for (int w = wv; w < W; w += NW) {
      const int n = n_live_w[w];
      if (lane < n) {
        const int slot = base_w[w] + lane;
        so[L.tok + slot] = g_tok[w][lane]; so[L.parent + slot] = g_prev[w][lane]; so[L.len + slot] = step_next + 1; so[L.win + slot] = w;
        so[L.win_slots + w * MAX_BEAMS + lane] = slot;
        s_tok[slot] = g_tok[w][lane]; s_par[slot] = g_prev[w][lane];
        ctl[B.slot + w * MB + lane] = slot;
        ctl[B.row_beam + slot] = lane;
      }
      if (lane == 0) so[L.win_nb + w] = n;
    }
  }
  // ---- the next step's rows: position tables copied from the parent's (double-buffered by step parity) and
  // x = E[token] + pos[len - 1] -- what dec_prepare_kernel does for a host-driven step
  if (a.x != nullptr && n_all > 0) {
    __syncthreads();
    int* tab_new = a.tabs + (size_t)(step_next & 1) * L.S * a.Lmax;
    const int* tab_old = a.tabs + (size_t)((step_next & 1) ^ 1) * L.S * a.Lmax;
    const int len = step_next + 1, d4 = a.d >> 2;
    if (len <= a.Lmax) {
      for (int r = wv; r < n_all; r += NW) {          // one wave per row
        const int parent = s_par[r], tk = s_tok[r];
        if (parent >= 0)
          for (int p = lane; p < len - 1; p += 64) tab_new[r * a.Lmax + p] = tab_old[parent * a.Lmax + p];
        if (lane == 0) tab_new[r * a.Lmax + len - 1] = step_next * L.S + r;
        const float4* e = reinterpret_cast<const float4*>(a.E + (int64_t)tk * a.d);
        const float4* pp = reinterpret_cast<const float4*>(a.pos + (int64_t)(len - 1) * a.d);
        float4* o = reinterpret_cast<float4*>(a.x + (int64_t)r * a.d);
        for (int c = lane; c < d4; c += 64) {
          const float4 u = e[c], v = pp[c];
          o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
        }
      }
    }
  }
}

#undef TSBEAM_SCAN

}  // namespace

void launch_dec_tsbeam_rows(hipStream_t st, const TsBeamRowsArgs& a, int n_rows) {
  WB_KLAUNCH(dec_tsbeam_rows_kernel, dim3(n_rows), dim3(TS_NT), 0, st, a);
}

void launch_dec_tsbeam_update(hipStream_t st, const TsBeamUpdateArgs& a) {
  WB_KLAUNCH(dec_tsbeam_update_kernel, dim3(1), dim3(1024), 0, st, a);
}

void launch_tsbeam_rows_hook(hipStream_t st, const TsBeamRowsHookArgs& a) {
  WB_KLAUNCH(tsbeam_rows_hook_kernel, dim3(a.R), dim3(TS_NT), 0, st, a);
}

}  // namespace wb
