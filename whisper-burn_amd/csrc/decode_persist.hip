// Persistent, flag-chained greedy decode: ONE co-resident grid runs every sublayer of every decode step.
//
// Why: with a handful of live rows a decode step is a chain of 3 n_layer + 2 dependent sublayers, each of which streams
// 0.2-0.6 MB of weights / cached K,V through ONE compute unit.  As separate launches (decode_fused.hip) every link pays its
// dispatch, a memory round trip for its input planes, and -- the largest term -- the time a single CU needs to pull the
// block's operands (~5 us of a ~10 us launch), none of which depends on the predecessor.  Here every role of a step is
// resident at once: a block issues the loads of its weights (and, for cross-attention, of the window's whole cached K)
// FIRST, then waits for the arrival counter of its producers, then folds their planes; the operand pull of sublayer
// k + 1 runs under sublayer k.  The reference recomputes the whole decoder per token (/root/reference/src/transcribe.rs:
// 253-307, src/model/mod.rs:345-350); the arithmetic of a step here is the arithmetic of the fused sublayer kernels
// (decode_fused_bodies.h: same device templates, same fixed summation orders -> bit-reproducible).
//
// Roles of one step, in dependency order:
//   per layer l: attn (head h, row r) x H R  ->  cross (h, r) x H R  ->  mlp (64-unit hidden slice j) x 4 d / 64
//   logits (a run of 128-column vocabulary tiles; each applies the final LayerNorm to the rows itself)   ->   merge (row r) x R
//   (WHISPER_HIP_PERSIST_MLP=planes, and any grid with fewer than 4 d / 64 blocks: a final-LN role (row r) x R in front of the
//   logits roles, ln(x + last MLP planes) once per row -- "the MLP edge" below)
// The host deals the roles to the blocks (decode_chain.cpp): a block runs its own list, in dependency order, every step.  The
// first sublayers' blocks take no logits work (they are back at their wait, weights requested, before the step ends).
// Dependencies = arrival counters (handoff.h), monotonic within the launch:
//   attn(0,.,r)  behind a step that chose its token: waits for that step's tile records of row r (tagged, below);
//                pre-wake on the GO word of epoch e and on c_x[r] >= e - 1.  Step 0, behind a prompt step, a row that ends,
//                WHISPER_HIP_PERSIST_PICK=merge: waits for merge(r) of the previous step (its x row)   c_x[r] >= e
//   cross(0,.,r) pre-wake: merge(r) of the previous step                       c_x[r]       >= e
//   attn(l,.,r)  pre-wake: the cross-attention blocks of layer l - 1; then the row's granules from the MLP roles of layer l - 1
//   cross(l,.,r) waits for the H attention blocks of its row                   c_attn[l][r] >= (e + 1) H
//   mlp(l,.)     waits for every cross-attention block of the layer            c_cross[l]   >= (e + 1) H R
//   logits(.)    pre-wake: the last layer's cross-attention blocks (GO words); then the rows' granules from its MLP roles
//   merge(r)     waits for every logits role (8 counters, role q arrives at q mod 8)  c_log[k] >= (e + 1) n_k
// Every block's list follows one global dependency order and all blocks are co-resident (the host sizes the grid from
// the occupancy query), so the smallest unfinished role can always run: no deadlock.  Reuse of the plane
// buffers across steps is ordered by the same chain (a role arrives only after its last read).
//
// The MLP edge.  An MLP role is split over the hidden dimension for both matrices.  In the `planes` form block j leaves a full-
// width partial of hid . W2 and every consumer block re-sums 4 d / 64 planes (77 KB swept per block at d = 384; a final-LN role per
// row does it once for the logits blocks).  Default, two phases (decode_fused_bodies.h: dec_mlp_body): block j publishes its 64
// hidden values per live row into g_hid [S][4 d] (tag = the role's tag_out), sweeps all 4 d of them -- no counter: the data is
// the flag -- and finishes the 16 residual columns [16 j, 16 j + 16) with the same sums, operand for operand and in the same
// order, that the planes and the consumers' folds went through; the columns go straight into the next stage's x stream as
// granules with tag_out.  attn(l + 1) takes the row as a finished stream (KSp = 0, the path layer 0 always used) and the logits
// roles sweep the last layer's rows and normalise them per wave (ps_finln_role's expression on the same operands): no planes, no
// plane bias on that edge, no stream store by slice 0, no final-LN stage.  The role arrives on c_mlp[l] behind phase 2.
//   * g_hid is ONE buffer for all layers and steps.  Its readers are the phase-2 sweeps of the stage that wrote it.  The next
//     writer is phase 1 of the next MLP stage (layer l + 1, or layer 0 of step e + 1); that stage runs behind cross(l + 1) <-
//     attn(l + 1) <- the finished row of a live row, which exists only when ALL 4 d / 64 blocks of stage l have published their
//     columns, i.e. behind their sweeps (a block publishes after its whole sweep, and a sweep's loads have returned when its
//     values are used).  Across the step boundary the same chain runs through logits -> records / merge -> attn(0).  No new
//     counter and no new tag value: a stale granule of g_hid carries another stage's tag.
//   * The x stream buffer the columns go to was last read by cross(l) (its attention stream); the MLP role has folded those
//     roles' planes before phase 1, so their reads are over -- the order slice 0's stream store relied on.
//   * Phase 2 waits for roles of the SAME stage, so the 4 d / 64 MLP roles of a layer must sit on different blocks ("the
//     smallest unfinished role can always run" would not hold otherwise): the host selects this form only on a grid of at least
//     4 d / 64 blocks (layer role i sits on block i % grid) and the `planes` form below that (decode_chain.cpp).
//   * x_fin, the rows the logits roles sweep, is overwritten by merge(r) of the same step (even layer counts: it is x0) -- behind
//     every logits arrival -- or by attn(0) of the next step (odd layer counts), which has seen every tile record of the row
//     or waited for merge(r); either way behind the logits roles' sweeps.  The final-LN role's read of x_fin was ordered the same way.
//
// The step boundary.  The logits roles leave one 16-byte record {tag, value, tag, id} per (row, tile), tagged with the step's
// final-LN tag, in the buffer of the step's parity.  attn(0,h,r) of step e sweeps row r's records of step e - 1, takes the argmax
// (`better`: a strict total order, so every block of the row gets merge(r)'s id), and builds E[tok] + pos[len] itself: two
// dependent round trips where the merge role's flag, its gather, its arrival and the x-row sweep were six.  merge(r) keeps
// all of its work (token row, gctl, dead flag, stop word, the x0 granules, the tables); nothing waits for it on this path.
// Ordering rules the edge keeps:
//   (a) every block's role list stays a subsequence of the global dependency order (ps_deal_roles is as it was);
//   (b) attn(0) of step e overwrites the attention planes and the folded stream that the cross-attention roles of step e - 1
//       read: the GO word of epoch e is stored by the LAST cross-attention arrival of step e - 1, so those reads are over;
//       cross(0,h,r) of step e writes the stream merge(r) of step e - 1 writes its x0 row into: it keeps its wait on
//       c_x[r] >= e, so the merge role's stores have drained before it stores;
//   (c) the records of parity p are rewritten by the logits roles of step e + 1; their readers are attn(0) of step e (ahead
//       of that write by the chain itself) and merge of step e - 1 (ahead because attn(0) of step e + 1 waited for c_x >= e,
//       that merge's arrival) -- hence two parities and the c_x word in the pre-wake;
//   (d) results depend on neither timing nor placement; every spin is bounded (HX_SPIN_LIMIT / HX_SWEEP_LIMIT), a give-up
//       sets the error word and the session falls back to the graph-replayed chain.
// A row that ends (its pick is eot, or no record compares) waits for merge(r) as before and finds its dead flag: every
// downstream role reads the dead flag and the stop word in the order it always did.
//
// End of the decode: the merge role of the last window to end stores HX_STOP = first step that must not run; every wait
// polls that word next to its counter, and a block that sees it leaves the kernel (without arriving).  Rows whose window
// has ended are marked dead: their attention roles skip the work and arrive at once.
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "decode.h"
#include "decode_fused_bodies.h"
#include "handoff.h"
#include "wave_ops.h"

namespace wb {
namespace {

using namespace fused;

constexpr int PS_NT = 512;
constexpr int PS_CT = 128;      // vocabulary columns per logits tile
constexpr int PS_NGO = 16;      // wake-up words of the logits roles (a few hundred pollers: ~13 per word)

// ---- final LayerNorm role: row r of  ln(x + b2 + sum_j P2[j])  (mod.rs:155), once per row ---------------------------------
// A few hundred logits blocks each folding the 4 d / 64 planes themselves pulled 22 MB through the fabric per step (write-
// through data is not shared through the L2s); one block per row folds and normalises, and the logits blocks read d values.
template <int DPL>
struct FinLnLds { alignas(16) float hs[64 * DPL]; };
template <int DPL>
__device__ __forceinline__ bool ps_finln_role(const PersistArgs& a, const int r, const PsStep& ps, FinLnLds<DPL>& sm) {
  constexpr int d = 64 * DPL, FP = 4 * DPL;
  auto& hs = sm.hs;
  const int tid = role_tid<true>(), lane = tid & 63, wave = tid >> 6;
  const int c = tid < d ? tid : 0;
  const float g_own = a.ln_g[c], b_own = a.ln_b[c];   // thread = column: every wave normalises its own 64 columns
  float accp = a.b2_last[c];
  if (!ps_wait(ps)) return false;                   // pre-wake: the last layer's cross-attention blocks have finished
  if (ld_i<true>(ps.dead + r) != 0) return true;
  ps_nap<2>();
  const Buf16 xgb(a.x_fin), pgb(a.P2);
  const uint32_t pvo = (uint32_t)(r * d + c);
  const int iplane = a.S * d;
  float v = 0.f;
  unsigned sweeps = 0;
  Gran gx{0u, 0.f}, g[FP];
#pragma unroll
  for (int j = 0; j < FP; j++) g[j] = Gran{0u, 0.f};
  for (;;) {
    if (gx.tag != ps.tag_in) gx = ld_gran(xgb, pvo, 0u);
#pragma unroll
    for (int j = 0; j < FP; j++)
      if (j < a.nb_mlp && g[j].tag != ps.tag_in) g[j] = ld_gran(pgb, pvo, (uint32_t)(j * iplane));
    bool ok = gx.tag == ps.tag_in;
#pragma unroll
    for (int j = 0; j < FP; j++) ok &= (j >= a.nb_mlp) || g[j].tag == ps.tag_in;
    if (ok) {
#pragma unroll
      for (int j = 0; j < FP; j++) accp += (j < a.nb_mlp) ? g[j].v : 0.f;             // s ascending (mod.rs:346-348)
      v = gx.v + accp;
      break;
    }
    if (ps_sweep_retry(sweeps, ps)) { *ps.lds_flag = 0; break; }
  }
  if (tid < d) hs[tid] = v;
  ps_stamp(ps, 2);
  __syncthreads();
  if (!ps_sweeps_ok(ps)) return false;
  if (wave < DPL) {                                 // (statistics per wave: no second barrier, no LDS round trip of the result)
    float mean, denom;
    ln_stats_lds<DPL>(hs, d, lane, a.ln_eps, a.ln_inside, mean, denom);
    const Buf16 xo(a.g_xn);
    st_gran(xo, (uint32_t)(r * d + tid), ps.tag_out, (v - mean) / denom * g_own + b_own);
  }
  return true;
}

// ---- logits role: tiles of  xn . E^T  (mod.rs:156), last position only ----------------------------------------------------
// Both E^T tiles of the role (d x 128 floats = d / 16 float4 per thread each) are in flight before the wait.  The
// rows arrive as granules: finished rows of the last layer's MLP roles, normalised here (a.mlp2), or rows already normalised
// by the final-LN roles (planes form).  Per row and tile the block leaves the best masked logit and its id --
// greedy needs the argmax only (log_softmax is monotone: transcribe.rs:276 with beam.rs k = 1).
template <int MR, int DPL>
struct LogitsLds {
  alignas(16) float xs[MR][64 * DPL];
  alignas(16) float xn[MR][64 * DPL];              // (final LayerNorm inside the role: every wave's own k-range of ln(xs))
  alignas(16) float red[8][MR][PS_CT];
  float tilev[MR][PS_CT];
};
template <int MR, int DPL>
__device__ __forceinline__ bool ps_logits_role(const PersistArgs& a, const int tile0, const int n_t, const PsStep& ps,
                                               const bool forced, const int par, LogitsLds<MR, DPL>& sm) {
  constexpr int d = 64 * DPL, NT = PS_NT, CT = PS_CT;
  constexpr int NR = d / 16;                        // E^T rows per thread: k = (2 wave + hh) NR + i
  constexpr int EPT = (MR * d + NT - 1) / NT;
  constexpr int PCH = EPT <= 3 ? 8 : EPT <= 6 ? 4 : 2;
  constexpr int NQ = MR * CT / NT;                  // tile values per thread in the column-sum pass
  constexpr bool TWO = DPL <= 6;                    // two tiles resident (2 x d / 16 float4 per thread) where they fit
  auto& xs = sm.xs; auto& red = sm.red; auto& tilev = sm.tilev;
  const int tid = role_tid<true>(), lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, c4 = (lane & 31) * 4;
  // a.mlp2: the rows arrive finished but not normalised (the last layer's MLP roles' columns); every wave takes the rows'
  // statistics itself and normalises the 2 NR columns its own E^T rows multiply -- ps_finln_role's expression on the same
  // operands, no barrier beyond the one behind the sweep.  Lane l < 2 NR owns column 2 wave NR + l
  const bool own_ln = a.mlp2 != 0;
  const int ln_col = 2 * wave * NR + (lane < 2 * NR ? lane : 0);
  float g_own = 0.f, b_own = 0.f;
  if (own_ln) { g_own = gld(a.ln_g + ln_col); b_own = gld(a.ln_b + ln_col); }
  // (buffer loads: one lane offset, the row offset i vocab_ld rides in the scalar offset -- 24 64-bit addresses per lane
  // would otherwise live across the tile loop)
  const Buf16 etb(a.Et);
  auto load_tile = [&](float4 (&w)[NR], int tile) {
    const int n0 = tile * CT;
    const bool col_ok = n0 + c4 < a.vocab_ld;      // lanes past the padded vocabulary re-read the tile's first columns
    const uint32_t vo = (uint32_t)((2 * wave + hh) * NR * a.vocab_ld + n0 + (col_ok ? c4 : 0));
#pragma unroll
    for (int i = 0; i < NR; i++) w[i] = ld_f4_plain(etb, vo, (uint32_t)(i * a.vocab_ld));
  };
  // Both tiles of the role are requested BEFORE the wait where the registers allow it: streamed after the wait, the
  // second tile of 203 blocks (40 MB at once, next to everybody's weight prefetch for the next step) took ~20 us
  // (profiles/r03_c_ps_timeline_phases.txt).
  float4 w0[NR], w1[TWO ? NR : 1];
  if (!forced) {                                    // (a prompt step chooses nothing: no E^T stream)
#if !defined(WB_PS_DRY)
    load_tile(w0, tile0);
    if constexpr (TWO) { if (n_t > 1) load_tile(w1, tile0 + 1); }
#endif
  }
  const int use_mask = (ps.step + 1 <= a.mask_until_len) ? 1 : 0;          // transcribe.rs:271-275
  int deadm = 0;                                    // bit r: row r takes no part (its window has ended)
  if (!ps_wait(ps)) return false;                   // pre-wake: the last layer's cross-attention blocks have finished
  // (no nap: the wake-up word reaches a few hundred pollers ~9 us after the broadcast -- the last MLP has finished by then)
  {
    // the rows (a.mlp2: finished, not yet normalised; else the final-LN roles' normalised ones): MR d granules, re-read until
    // every live row carries the producing stage's tag
    int off[EPT];
#pragma unroll
    for (int i = 0; i < EPT; i++) {
      int e = tid + NT * i;
      if (e >= MR * d) e = tid;
      off[i] = e;
    }
#pragma unroll
    for (int r = 0; r < MR; r++)
      if (r >= ps.n_rows || ld_i<true>(ps.dead + min(r, ps.n_rows - 1)) != 0) deadm |= 1 << r;
    const Buf16 xgb(own_ln ? a.x_fin : a.g_xn);
    float v[EPT];
    unsigned sweeps = 0;
    for (;;) {
      Gran gx[EPT];
#pragma unroll
      for (int i = 0; i < EPT; i++) gx[i] = ld_gran(xgb, (uint32_t)off[i], 0u);
      bool ok = true;
#pragma unroll
      for (int i = 0; i < EPT; i++) ok &= ((deadm >> (off[i] / d)) & 1) != 0 || gx[i].tag == ps.tag_in;
      if (ok) {
#pragma unroll
        for (int i = 0; i < EPT; i++) v[i] = ((deadm >> (off[i] / d)) & 1) ? 0.f : gx[i].v;
        break;
      }
      if (ps_sweep_retry(sweeps, ps)) { *ps.lds_flag = 0; break; }
    }
#pragma unroll
    for (int i = 0; i < EPT; i++) {
      const int e = tid + NT * i;
      if (e < MR * d) (&xs[0][0])[e] = v[i];
    }
  }
  ps_stamp(ps, 2);
  __syncthreads();
  if (!ps_sweeps_ok(ps)) return false;
  ps_stamp(ps, 3);
  // a prompt step: the role has kept its place in the chain (it arrives after the rows' producers, the merge role after it --
  // the order the reuse of the x rows and planes relies on) and is done
  if (forced) return true;
  const float (*xg)[d] = xs;                        // what the GEMV multiplies
#if !defined(WB_PS_DRY)
  if (own_ln) {
#pragma unroll
    for (int r = 0; r < MR; r++) {
      if ((deadm >> r) & 1) continue;
      float mean, denom;
      ln_stats_lds<DPL>(xs[r], d, lane, a.ln_eps, a.ln_inside, mean, denom);
      if (lane < 2 * NR) sm.xn[r][ln_col] = (xs[r][ln_col] - mean) / denom * g_own + b_own;
    }
    __builtin_amdgcn_wave_barrier();                // (a wave reads back only the columns its own lanes wrote)
    xg = sm.xn;
  }
#endif
#if defined(WB_PS_DRY)
  // dry build (tools/build_exp.sh dry): the role's tile records without the E^T stream and the GEMV -- token 0-ish every step
  for (int t = 0; t < n_t; t++)
    if (wave < MR && !((deadm >> wave) & 1)) {
      const int r_u = __builtin_amdgcn_readfirstlane(wave);
      if (lane == 0) st_rec(Buf16(a.tstats), (uint32_t)((par * a.S + r_u) * a.n_tiles + tile0 + t), ps.tag_in, 0.f, (tile0 + t) * CT);
    }
  return true;
#endif
  // one tile: GEMV from the registers, column sums over the eight waves, mask, per-row best (value desc, id asc)
  auto run_tile = [&](const float4 (&w)[NR], int tile) {
    const int n0 = tile * CT;
    float mk[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int col = n0 + ((tid + NT * q) & (CT - 1));
      mk[q] = (use_mask && col < a.V) ? a.mask[col] : 0.f;
    }
    float acc[MR][4];
#pragma unroll
    for (int r = 0; r < MR; r++) { acc[r][0] = acc[r][1] = acc[r][2] = acc[r][3] = 0.f; }
#pragma unroll
    for (int r = 0; r < MR; r++) {
      if ((deadm >> r) & 1) continue;               // (rows whose window has ended cost nothing)
#pragma unroll
      for (int i4 = 0; i4 < NR; i4 += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(&xg[r][(2 * wave + hh) * NR + i4]);
        acc[r][0] += xv.x * w[i4].x; acc[r][1] += xv.x * w[i4].y; acc[r][2] += xv.x * w[i4].z; acc[r][3] += xv.x * w[i4].w;
        acc[r][0] += xv.y * w[i4 + 1].x; acc[r][1] += xv.y * w[i4 + 1].y; acc[r][2] += xv.y * w[i4 + 1].z; acc[r][3] += xv.y * w[i4 + 1].w;
        acc[r][0] += xv.z * w[i4 + 2].x; acc[r][1] += xv.z * w[i4 + 2].y; acc[r][2] += xv.z * w[i4 + 2].z; acc[r][3] += xv.z * w[i4 + 2].w;
        acc[r][0] += xv.w * w[i4 + 3].x; acc[r][1] += xv.w * w[i4 + 3].y; acc[r][2] += xv.w * w[i4 + 3].z; acc[r][3] += xv.w * w[i4 + 3].w;
      }
    }
#pragma unroll
    for (int r = 0; r < MR; r++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[r][c] = xor32_sum(acc[r][c]);        // the two row halves of the wave
    __syncthreads();                                // (the previous tile's readers of red / tilev are done)
    if (hh == 0) {
#pragma unroll
      for (int r = 0; r < MR; r++)
        *reinterpret_cast<float4*>(&red[wave][r][c4]) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int e = tid + NT * q, r = e / CT, c = e & (CT - 1);
      float v = 0.f;
#pragma unroll
      for (int w8 = 0; w8 < 8; w8++) v += red[w8][r][c];
      v += mk[q];
      if (n0 + c >= a.V) v = -INFINITY;
      tilev[r][c] = v;
    }
    __syncthreads();
    if (wave < MR && !((deadm >> wave) & 1)) {
      const int r = wave;
      const float v0 = tilev[r][lane], v1 = tilev[r][lane + 64];
      float bvv; int bi;
      if (better(v0, lane, v1, lane + 64)) { bvv = v0; bi = lane; } else { bvv = v1; bi = lane + 64; }
      wave_argmax(bvv, bi);
      // this step's record of (row, tile): parity `par`, tagged with the step's final-LN tag, ONE 16-byte write-through store
      // (the wave-uniform row is taken by the whole wave, in front of the one-lane branch: a wave operation of lane 0 alone
      // would meet the other lanes' next one)
      const int r_u = __builtin_amdgcn_readfirstlane(r);
      if (lane == 0) st_rec(Buf16(a.tstats), (uint32_t)((par * a.S + r_u) * a.n_tiles + tile), ps.tag_in, bvv, n0 + bi);
    }
  };
  run_tile(w0, tile0);
  ps_stamp(ps, 4);
  if constexpr (TWO) {
    if (n_t > 1) run_tile(w1, tile0 + 1);
    ps_stamp(ps, 5);
    for (int t = 2; t < n_t; t++) { load_tile(w0, tile0 + t); run_tile(w0, tile0 + t); }
  } else {
    for (int t = 1; t < n_t; t++) { load_tile(w0, tile0 + t); run_tile(w0, tile0 + t); }
  }
  return true;
}

// ---- merge role: row r's argmax over the tiles, the chain's bookkeeping, the next step's embedding -------------------
// (what dec_topk_merge_kernel + chained_update do between two launches; transcribe.rs:235-241 for the end of a row)
struct MergeLds { float redv[8]; int redi[8]; unsigned tgt[8]; };
__device__ __forceinline__ bool ps_merge_role(const PersistArgs& a, const int r, const int e, const PsStep& ps0,
                                              const unsigned* clog, const int* n_per_ctr, MergeLds& sm) {
  auto& redv = sm.redv; auto& redi = sm.redi;
  const int tid = role_tid<true>(), lane = tid & 63, wave = tid >> 6;
  const PsStep& ps = ps0;
  {
    // every logits role of this step has arrived (8 sharded counters, polled by 8 lanes at once)
    auto& tgt = sm.tgt;
    if (tid < 8) tgt[tid] = (unsigned)(e + 1) * (unsigned)n_per_ctr[tid];
    __syncthreads();
    if (!hx_wait_many(clog, tgt, 8, ps.ctl, ps.step, 1000, ps.lds_flag)) return false;
  }
  ps_stamp(ps, 1);
  const int len = ps.step + 1;                      // tokens in the row so far; the new one lands at index len
  const int fin_now = ld_i<true>(a.dead + r);
  const int tok_prev = ld_i<true>(a.gctl + GC_HDR + r);
  int gi;
  if (e < a.n_forced) {
    gi = a.forced[e];                               // prompt prefill: the next position holds the next prompt token
  } else {
    float bv = -INFINITY; int bi = 0x7fffffff;
    // (the counters above say every record of this step is in memory: the tags are the first-layer self-attention roles')
    const Buf16 recb(a.tstats);
    for (int t = tid; t < a.n_tiles; t += PS_NT) {
      const Rec q = ld_rec(recb, (uint32_t)(((e & 1) * a.S + r) * a.n_tiles + t));
      if (better(q.v, q.id, bv, bi)) { bv = q.v; bi = q.id; }
    }
    wave_argmax(bv, bi);
    if (lane == 0) { redv[wave] = bv; redi[wave] = bi; }
    __syncthreads();
    float gv = redv[0]; gi = redi[0];
#pragma unroll
    for (int j = 1; j < 8; j++)
      if (better(redv[j], redi[j], gv, gi)) { gv = redv[j]; gi = redi[j]; }
    // no finite candidate (NaN logits): never an embedding index -- the row ends, the host fails the call (decode.hip: top1_or_eot)
    if ((unsigned)gi >= 0x7fffffffu) { gi = a.eot; if (tid == 0) a.gctl[GC_BAD] = 1; }
  }
  const int finished = fin_now || (gi == a.eot && e >= a.n_forced);
  const int tok_next = fin_now ? tok_prev : gi;     // a finished row keeps its last token (its later argmax is stale)
  if (tid == 0 && !fin_now) {
    st_i_sc1(a.gctl + GC_HDR + r, gi);
    a.gtok[r * a.Lmax + len] = gi;
    a.gctl[GC_HDR + 2 * a.S + r] = len + 1;
    if (gi == a.eot && e >= a.n_forced) {           // transcribe.rs:235-241: the row has ended
      a.gctl[GC_HDR + a.S + r] = 1;
      st_i_sc1(a.dead + r, 1);
      const unsigned n = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(a.ctl + HX_NDONE), 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT) + 1u;
      if ((int)n == ps.n_rows) st_i_sc1(a.ctl + HX_STOP, ps.step + 1);     // every window has ended: no further step
    }
  }
  if (tid == 0 && r == 0) a.gctl[GC_STEP] = ps.step + 1;
  if (len < a.Lmax) {
    // next step: position len holds tok_next -> x0[r] = E[tok_next] + pos[len] (mod.rs:141-146); position tables
    const Buf16 xb(a.x0);
    const float4* ev = reinterpret_cast<const float4*>(a.E + (int64_t)tok_next * a.d);
    const float4* pp = reinterpret_cast<const float4*>(a.pos + (int64_t)len * a.d);
    const unsigned tag_x = a.tag_base + 1u + 3u * (unsigned)((e + 1) * a.n_layer);   // what attn(0) of step e + 1 expects
    for (int c = tid; c < (a.d >> 2); c += PS_NT) {
      const float4 x = ev[c], y = pp[c];
      st_gran4(xb, (uint32_t)(r * a.d + 4 * c), tag_x, make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w));
    }
    // (the persistent roles address the self-attention cache arithmetically; the tables are kept for host-driven steps
    // that may follow the chain)
    const int nstep = ps.step + 1;
    int* tab_new = a.tabs + (size_t)(nstep & 1) * a.S * a.Lmax;
    for (int p = tid; p <= len; p += PS_NT) tab_new[r * a.Lmax + p] = p * a.S + r;
  }
  (void)finished;
  return true;
}

// ---- the grid ---------------------------------------------------------------------------------------------------------
// One LDS arena per block: the roles' arrays share one union (a block runs its roles one after another), the wait's
// broadcast word follows, and what is left of the CU's 160 KB holds the resident operands of a block whose role list has
// exactly one layer role, a self- or cross-attention one (decode_fused_bodies.h: ResGeom) -- whole per-thread float4 slots.
template <int DPL, int MR, int NP>
union PsRoleLds {
  MlpLds<MR, DPL, false> mlp; AttnLds<DPL> attn; CrossLds<DPL, NP> cross;
  FinLnLds<DPL> finln; LogitsLds<MR, DPL> logits; MergeLds merge;
};
constexpr int PS_LDS_BYTES = 160 * 1024;
// (d >= 384 with 8 rows or with the two-pass key ring keeps the streamed path: those instances sit hardest at the register
// limit, and with the resident path compiled in each spilled one dword more than before)
constexpr bool ps_resident_instance(int DPL, int MR, int NP) { return !(DPL >= 6 && (MR == 8 || NP == 2)); }
template <int DPL, int MR, int NP>
struct PsArena {
  static constexpr int ROLE_BYTES = (int)((sizeof(PsRoleLds<DPL, MR, NP>) + 15) / 16 * 16);
  static constexpr int FLAG_BYTES = 16;             // wait_flag, padded: the resident region stays 16-byte aligned
  static constexpr int RS = ps_resident_instance(DPL, MR, NP) ? (PS_LDS_BYTES - ROLE_BYTES - FLAG_BYTES) / (PS_NT * 16) : 0;   // resident float4 slots per thread
  static constexpr int BYTES = ROLE_BYTES + FLAG_BYTES + RS * PS_NT * 16;   // each of the three objects padded to 16 bytes
  static_assert(RS >= 0 && BYTES <= PS_LDS_BYTES, "the persistent kernel's LDS arena exceeds 160 KB");
  // (does anything useful fit?)
  static constexpr bool USEFUL = ResGeom<DPL, NP, RS>::WO_A + ResGeom<DPL, NP, RS>::NWO_A + ResGeom<DPL, NP, RS>::WO_X +
                                 ResGeom<DPL, NP, RS>::NWO_X > 0;
};
static_assert(PS_NT == ROLE_NT, "block size");
#define WB_PS_INSTANCES(X) X(2, 4, 1) X(2, 8, 1) X(6, 4, 1) X(6, 8, 1) X(8, 4, 1) X(2, 4, 2) X(6, 4, 2) X(8, 4, 2)
#define WB_PS_CHECK(DPL_, MR_, NP_) static_assert(PsArena<DPL_, MR_, NP_>::BYTES <= 160 * 1024, "LDS arena of an instance");
WB_PS_INSTANCES(WB_PS_CHECK)
#undef WB_PS_CHECK

template <int DPL, int MR, int NP>
__global__ __launch_bounds__(PS_NT) void dec_persist_kernel(PersistArgs a) {
  using AR = PsArena<DPL, MR, NP>;
  constexpr int RS = AR::RS;
  // (three objects, not one struct: as members of one struct the bench instance spilled 36 B per lane instead of 20.  The
  // compiler may pack them a few bytes tighter than AR::BYTES, which pads each to 16: the asserted number is an upper bound)
  __shared__ PsRoleLds<DPL, MR, NP> lds;
  __shared__ __attribute__((aligned(16))) int wait_flag[AR::FLAG_BYTES / 4];
  __shared__ __attribute__((aligned(16))) float4 res_buf[RS > 0 ? RS * PS_NT : 1];
  static_assert(sizeof(lds) <= AR::ROLE_BYTES && sizeof(wait_flag) == AR::FLAG_BYTES && sizeof(res_buf) <= (RS > 0 ? RS : 1) * PS_NT * 16 &&
                AR::BYTES + (RS > 0 ? 0 : 16) <= PS_LDS_BYTES, "the three LDS objects are what PsArena accounts for");
  const int NL = a.n_layer, S = a.S, R = a.n_rows, H = a.n_head, NB = a.nb_mlp;
  // arrival counter c lives at ctl[HX_HDR + c HX_LINE]: one 128-byte line each
  auto cptr = [&](int c) { return reinterpret_cast<unsigned*>(a.ctl + HX_HDR + c * HX_LINE); };
  const int C_X = 0, C_ATTN = S, C_CROSS = S + NL * S, C_MLP = C_CROSS + NL, C_LOG = C_MLP + NL, C_GO = C_LOG + 8;
  int n_per_ctr[8];
#pragma unroll
  for (int k = 0; k < 8; k++) n_per_ctr[k] = (a.n_logits_roles + 7 - k) / 8;
  const int i_lo = a.role_off[blockIdx.x], i_hi = a.role_off[blockIdx.x + 1];
  // resident operands: the host names the role of a block whose ONE layer role is a self- or cross-attention role
  // (res_role); loaded once, here -- the weights are constant and the window's cached cross V is constant for the launch
#if defined(WB_PS_DRY)                              // (dry build: no operand loads at all)
  constexpr bool RES = false;
#else
  constexpr bool RES = RS > 0;
#endif
  int res_i = -1;
  if (RES && a.res_role != nullptr) res_i = a.res_role[blockIdx.x];
  if (res_i >= i_lo && res_i < i_hi) {
    const PsRole role = a.roles[res_i];
    if (role.kind == PSR_ATTN) dec_attn_res_fill<DPL, RS>(a.layers[role.layer].attn, role.a, res_buf);
    else if (role.kind == PSR_CROSS) dec_cross_res_fill<DPL, NP, RS>(a.layers[role.layer].cross, role.a, role.b, res_buf);
  }
  unsigned long long dead_seen = 0;                 // bit k: role i_lo + k of this block has found its row dead (it stays dead)
  for (int e = 0; e < a.n_steps; e++) {
    for (int i = i_lo; i < i_hi; i++) {
      const PsRole role = a.roles[i];
      PsStep ps;
      ps.known_dead = i - i_lo < 64 && ((dead_seen >> (i - i_lo)) & 1ull) != 0;
      ps.ctl = a.ctl; ps.step = a.step0 + e; ps.n_rows = R; ps.dead = a.dead; ps.lds_flag = &wait_flag[0];
      unsigned long long* stp = a.stamps ? a.stamps + ((size_t)e * a.n_roles + i) * PS_STAMPS : nullptr;
      if (stp && threadIdx.x == 0) stp[0] = wall_clock64();
      ps.stamp = stp;
      int out;
      bool ok;
      // granule tags: a stage's planes and folded stream carry tag(e, layer, sublayer); a role consumes tag - 1
      const unsigned tag_l = a.tag_base + 2u + 3u * (unsigned)(e * NL + (role.kind <= PSR_MLP ? role.layer : NL - 1));
      // step e - 1 chose its token (it was no prompt step) and this step's position row exists: the pick edge
      const bool pick_e = a.pick != 0 && e >= 1 && e - 1 >= a.n_forced && ps.step < a.Lmax;
      if (role.kind == PSR_ATTN) {
        AttnFusedArgs la = a.layers[role.layer].attn;
        if (a.mlp2) { la.KSp = 0; ps.x_late = role.layer > 0; }   // (the previous layer's MLP roles left the finished row: nothing to fold)
        // layer 0: the merge role's flag (its x row follows as granules); else pre-wake = the previous layer's
        // cross-attention blocks have finished (its MLP, the producer, is running)
        if (role.layer == 0) { ps.ctr_index = C_X + role.b; ps.target = (unsigned)e; }
        else { ps.ctr_index = C_CROSS + role.layer - 1; ps.target = (unsigned)(e + 1) * H * R; }
        ps.ctr = cptr(ps.ctr_index);
        ps.tag_out = tag_l; ps.tag_in = tag_l - 1u;
        if (role.layer == 0 && pick_e) {             // the step boundary: the role picks the row's token from the records itself
          ps.pk_rec = static_cast<const char*>(a.tstats) + ((size_t)((e - 1) & 1) * S + role.b) * a.n_tiles * sizeof(Rec);
          ps.pk_n_tiles = a.n_tiles;
          ps.pk_tag = a.tag_base + 4u + 3u * (unsigned)((e - 1) * NL + NL - 1);   // the final-LN tag of step e - 1
          ps.pk_go = cptr(C_GO + (role.b * H + role.a) % PS_NGO); ps.pk_go_target = (unsigned)e;
          ps.pk_E = a.E; ps.pk_pos = a.pos + (int64_t)ps.step * a.d; ps.pk_eot = a.eot;
        }
        ok = dec_attn_body<DPL, true, RS>(la, role.a, role.b, ps, lds.attn, i == res_i ? res_buf : nullptr);
        out = C_ATTN + role.layer * S + role.b;
      } else if (role.kind == PSR_CROSS) {
        const CrossFusedArgs la = a.layers[role.layer].cross;
        // pre-wake = the stage before the self-attention blocks: the previous layer's MLP (layer 0: the merge role)
        if (role.layer == 0) { ps.ctr_index = C_X + role.b; ps.target = (unsigned)e; }
        else { ps.ctr_index = C_MLP + role.layer - 1; ps.target = (unsigned)(e + 1) * NB; }
        ps.ctr = cptr(ps.ctr_index);
        ps.tag_out = tag_l + 1u; ps.tag_in = tag_l;
        ps.cross_early = role.layer == 0 && pick_e;
        ps.x_late = a.mlp2 != 0 && role.layer > 0;   // (its pre-wake, the previous layer's MLP roles' arrival, comes later)
        ok = dec_cross_body<DPL, true, NP, RS>(la, role.a, role.b, ps, lds.cross, i == res_i ? res_buf : nullptr);
        out = C_CROSS + role.layer;
      } else if (role.kind == PSR_MLP) {
        const MlpFusedArgs la = a.layers[role.layer].mlp;
        // pre-wake = the self-attention blocks of every row have finished (the cross-attention blocks are running)
        ps.ctr_index = C_ATTN + role.layer * S; ps.target = (unsigned)(e + 1) * H; ps.n_ctr = R;
        ps.ctr = cptr(ps.ctr_index);
        ps.tag_out = tag_l + 2u; ps.tag_in = tag_l + 1u;
        if (a.mlp2) {
          ps.mlp_hid = a.g_hid;
          ps.mlp_b2 = a.layers[role.layer].mlp_b2;
        }
        ok = dec_mlp_body<MR, DPL, false, true>(la, role.a, ps, lds.mlp);
        out = C_MLP + role.layer;
      } else if (role.kind == PSR_FINLN) {
        ps.ctr_index = C_CROSS + NL - 1; ps.target = (unsigned)(e + 1) * H * R;
        ps.ctr = cptr(ps.ctr_index);
        ps.tag_in = tag_l + 2u; ps.tag_out = tag_l + 2u;
        ok = ps_finln_role<DPL>(a, role.b, ps, lds.finln);
        out = C_GO + PS_NGO;                         // (nobody waits for it: the logits roles watch the granules)
      } else if (role.kind == PSR_LOGITS) {
        // a few hundred blocks: pre-woken by the last cross-attention block of the step through one of PS_NGO words; they
        // nap, then watch d granules per row -- the last layer's finished rows, or the final-LN roles' (a sweep of all 4 d / 64
        // MLP planes by every logits block was 22 MB per round: profiles/r03_c_ps_timeline_granules_v1.txt)
        ps.ctr_index = C_GO + (role.layer % PS_NGO); ps.target = (unsigned)(e + 1);
        ps.ctr = cptr(ps.ctr_index);
        ps.tag_in = tag_l + 2u;
        ok = ps_logits_role<MR, DPL>(a, role.a, role.b, ps, e < a.n_forced, e & 1, lds.logits);
        out = C_LOG + (role.layer & 7);
      } else {
        ok = ps_merge_role(a, role.b, e, ps, cptr(C_LOG), n_per_ctr, lds.merge);
        out = C_X + role.b;
      }
      if (!ok) return;                               // the decode was stopped (or a wait gave up): leave
      if (ps.saw_dead && i - i_lo < 64) dead_seen |= 1ull << (i - i_lo);
      if (stp && threadIdx.x == 0) stp[6] = wall_clock64();
      if (role.kind == PSR_CROSS && role.layer == NL - 1)
        hx_arrive_broadcast(cptr(out), (unsigned)(e + 1) * H * R, cptr(C_GO), PS_NGO, (unsigned)(e + 1));
      else
        hx_arrive(cptr(out));
      if (stp && threadIdx.x == 0) stp[7] = wall_clock64();
    }
  }
}

// the first step's x rows (dec_prepare_kernel wrote plain floats) as granules with the tag attn(0) of step 0 expects; the
// launch's stop word starts at "never" (the rest of the control block was zeroed on the stream in front of this kernel)
__global__ void ps_seed_kernel(const float* __restrict__ x, int n, void* gx, unsigned tag, int* ctl) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ctl[HX_STOP] = INT_MAX;
  const Buf16 b(gx);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) st_gran(b, (uint32_t)i, tag, x[i]);
}

// test-only (tools/kernel_harness.cpp: wbk_persist_pick): ps_pick_token as the first-layer self-attention role calls it, alone
__global__ __launch_bounds__(PS_NT) void ps_pick_test_kernel(const void* rec, int n_tiles, unsigned tag, int* ctl, int* out_id) {
  __shared__ float xch[16];
  __shared__ int flag;
  PsStep ps;
  ps.ctl = ctl; ps.step = -1; ps.lds_flag = &flag;   // (step -1: the zeroed stop word stops nothing)
  if (threadIdx.x == 0) flag = 1;
  __syncthreads();
  const int tok = ps_pick_token(rec, n_tiles, tag, ps, xch, role_tid<true>());
  if (threadIdx.x == 0) *out_id = ps_sweeps_ok(ps) ? tok : -1;
}

// test-only (tools/kernel_harness.cpp: wbk_persist_mlp2): the MLP roles of one layer in the two-phase form, block j = slice j
template <int DPL>
__global__ __launch_bounds__(PS_NT) void ps_mlp2_test_kernel(PsMlp2TestArgs t) {
  __shared__ MlpLds<4, DPL, false> sm;
  __shared__ int flag;
  PsStep ps;
  ps.ctl = t.ctl; ps.step = -1; ps.lds_flag = &flag;   // (step -1: the zeroed stop word stops nothing)
  ps.ctr = reinterpret_cast<const unsigned*>(t.ctl + HX_HDR); ps.target = 0u;   // (the wait is passed at once)
  ps.n_rows = t.n_rows; ps.dead = t.dead;
  ps.tag_in = t.tag_in; ps.tag_out = t.tag_in + 1u;
  ps.mlp_hid = t.g_hid; ps.mlp_b2 = t.b2;
  dec_mlp_body<4, DPL, false, true>(t.a, blockIdx.x, ps, sm);
}

// test-only (tools/kernel_harness.cpp: wbk_persist_logits): one logits role, behind the final-LN roles of its rows in the planes form
template <int DPL>
struct PsLogitsTestLds { union { FinLnLds<DPL> finln; LogitsLds<4, DPL> logits; }; };
struct PsLogitsTestArgs { PersistArgs a; unsigned tag; int n_t; };
template <int DPL>
__global__ __launch_bounds__(PS_NT) void ps_logits_test_kernel(PsLogitsTestArgs t) {
  const PersistArgs& a = t.a;
  const unsigned tag = t.tag;
  const int n_t = t.n_t;
  __shared__ PsLogitsTestLds<DPL> sm;
  __shared__ int flag;
  PsStep ps;
  ps.ctl = a.ctl; ps.step = -1; ps.lds_flag = &flag;   // (step -1: the zeroed stop word stops nothing; a.mask_until_len < 0: no mask)
  ps.ctr = reinterpret_cast<const unsigned*>(a.ctl + HX_HDR); ps.target = 0u;   // (every wait is passed at once)
  ps.n_rows = a.n_rows; ps.dead = a.dead;
  ps.tag_in = tag; ps.tag_out = tag;
  if (blockIdx.x == 0) {                             // block 0: the rows' final-LN roles (planes form); block 1: the logits role
    if (a.mlp2 == 0)
      for (int r = 0; r < a.n_rows; r++)
        if (!ps_finln_role<DPL>(a, r, ps, sm.finln)) return;
    return;
  }
  ps_logits_role<4, DPL>(a, 0, n_t, ps, false, 0, sm.logits);
}

template <int DPL, int MR, int NP>
int max_blocks_per_cu() {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (dec_persist_kernel<DPL, MR, NP>), PS_NT, 0) != hipSuccess) return 0;
  return nb;
}

}  // namespace

// resident float4 slots per thread of the instance that serves (d, n_rows, max_keys); 0: none, or nothing useful fits
int dec_persist_resident_slots(int d, int n_rows, int max_keys) {
  if (!dec_persist_supported(d, n_rows, max_keys)) return 0;
  const int dpl = d / 64, mr = n_rows > 4 ? 8 : 4, np = max_keys > CROSS_FUSED_MAX_C ? 2 : 1;
#define WB_PS_SLOTS(DPL_, MR_, NP_) \
  if (dpl == DPL_ && mr == MR_ && np == NP_) return PsArena<DPL_, MR_, NP_>::USEFUL ? PsArena<DPL_, MR_, NP_>::RS : 0;
  WB_PS_INSTANCES(WB_PS_SLOTS)
#undef WB_PS_SLOTS
  return 0;
}

// the resident geometry of that instance: out = {RS, NRND, NWO_A, NVT, NWO_X} (decode_fused_bodies.h: ResGeom); false: no instance
bool dec_persist_resident_geometry(int d, int n_rows, int max_keys, int out[5]) {
  if (!dec_persist_supported(d, n_rows, max_keys)) return false;
  const int dpl = d / 64, mr = n_rows > 4 ? 8 : 4, np = max_keys > CROSS_FUSED_MAX_C ? 2 : 1;
#define WB_PS_GEOM(DPL_, MR_, NP_)                                                            \
  if (dpl == DPL_ && mr == MR_ && np == NP_) {                                                \
    using RG = ResGeom<DPL_, NP_, PsArena<DPL_, MR_, NP_>::RS>;                               \
    out[0] = PsArena<DPL_, MR_, NP_>::RS; out[1] = RG::NRND; out[2] = RG::NWO_A; out[3] = RG::NVT; out[4] = RG::NWO_X; \
    if (PsArena<DPL_, MR_, NP_>::RS == 0) out[1] = out[2] = out[3] = out[4] = 0;              \
    return true;                                                                              \
  }
  WB_PS_INSTANCES(WB_PS_GEOM)
#undef WB_PS_GEOM
  return false;
}

int ps_ctl_ints(int S, int n_layer) { return HX_HDR + (S + n_layer * S + 2 * n_layer + 8 + PS_NGO + 1) * HX_LINE; }

// The shapes the kernel is instantiated for: d = 128 / 384 with up to 8 rows, d = 512 with up to 4, two key passes (768 < C <=
// 1536 keys: the opt-in 30 s window) with up to 4 rows.  (The limits date from the time every role's LDS was allocated side by
// side; with the roles in one union LDS no longer sets them, but the other shapes are not instantiated or tested.)
bool dec_persist_supported(int d, int n_rows, int max_keys) {
  if (n_rows < 1 || n_rows > 8) return false;
  if (max_keys > CROSS_FUSED_MAX_PASSES * CROSS_FUSED_MAX_C) return false;
  if (max_keys > CROSS_FUSED_MAX_C && n_rows > 4) return false;
  if (d == 128 || d == 384) return true;
  return d == 512 && n_rows <= 4;
}

int dec_persist_max_grid(int device, int d, int n_rows, int max_keys) {
  if (!dec_persist_supported(d, n_rows, max_keys)) return 0;
  int cus = 0, coop = 0;
  if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device) != hipSuccess || !coop) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return 0;
  int per = 0;
  const bool big = n_rows > 4;
  if (max_keys > CROSS_FUSED_MAX_C)
    per = d == 128 ? max_blocks_per_cu<2, 4, 2>() : d == 384 ? max_blocks_per_cu<6, 4, 2>() : max_blocks_per_cu<8, 4, 2>();
  else if (d == 128) per = big ? max_blocks_per_cu<2, 8, 1>() : max_blocks_per_cu<2, 4, 1>();
  else if (d == 384) per = big ? max_blocks_per_cu<6, 8, 1>() : max_blocks_per_cu<6, 4, 1>();
  else per = max_blocks_per_cu<8, 4, 1>();
  if (per <= 0) return 0;
  // (one block per CU is what the roles are sized for; a second resident block per CU would only share its fill path)
  return cus * 1;
}

void launch_ps_seed(hipStream_t st, const float* x, int n, void* gx, unsigned tag, int* ctl) {
  hipLaunchKernelGGL(ps_seed_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, n, gx, tag, ctl);
}

void launch_ps_pick_test(hipStream_t st, const void* rec, int n_tiles, unsigned tag, int* ctl, int* out_id) {
  hipLaunchKernelGGL(ps_pick_test_kernel, dim3(1), dim3(PS_NT), 0, st, rec, n_tiles, tag, ctl, out_id);
}

int launch_ps_mlp2_test(hipStream_t st, const PsMlp2TestArgs& t) {
  if ((t.a.d != 128 && t.a.d != 384) || t.n_rows < 1 || t.n_rows > 4 || t.n_rows > t.a.S) return -1;
  const dim3 g(4 * t.a.d / 64), b(PS_NT);
  hipError_t e;
  if (t.a.d == 128) e = WB_LAUNCH_COOP((ps_mlp2_test_kernel<2>), g, b, 0, st, t);
  else e = WB_LAUNCH_COOP((ps_mlp2_test_kernel<6>), g, b, 0, st, t);
  return e == hipSuccess ? 0 : -1;
}

int launch_ps_logits_test(hipStream_t st, const PersistArgs& a, unsigned tag, int n_t) {
  if ((a.d != 128 && a.d != 384) || a.n_rows < 1 || a.n_rows > 4 || a.n_rows > a.S || n_t < 1 || n_t > 2 || n_t > a.n_tiles) return -1;
  // (a cooperative launch like the kernel it stands for: the roles nap and re-read, which the functional model allows only there)
  const PsLogitsTestArgs t{a, tag, n_t};
  const dim3 g(2), b(PS_NT);
  const hipError_t e = a.d == 128 ? WB_LAUNCH_COOP((ps_logits_test_kernel<2>), g, b, 0, st, t) : WB_LAUNCH_COOP((ps_logits_test_kernel<6>), g, b, 0, st, t);
  return e == hipSuccess ? 0 : -1;
}

int launch_dec_persist(hipStream_t st, const PersistArgs& a, int grid) {
  const dim3 g(grid), b(PS_NT);
  const bool big = a.n_rows > 4;
  hipError_t e = hipErrorInvalidValue;
#define WB_PS(DPL_, MR_, NP_) e = WB_LAUNCH_COOP((dec_persist_kernel<DPL_, MR_, NP_>), g, b, 0, st, a)
  if (a.n_pass > 1) {
    if (big) return -1;
    if (a.d == 128) WB_PS(2, 4, 2); else if (a.d == 384) WB_PS(6, 4, 2); else if (a.d == 512) WB_PS(8, 4, 2);
  }
  else if (a.d == 128) { if (big) WB_PS(2, 8, 1); else WB_PS(2, 4, 1); }
  else if (a.d == 384) { if (big) WB_PS(6, 8, 1); else WB_PS(6, 4, 1); }
  else if (a.d == 512 && !big) WB_PS(8, 4, 1);
#undef WB_PS
  return e == hipSuccess ? 0 : -1;
}

}  // namespace wb
