// Temperature sampling: one Gumbel-max draw per (row, step) on a counter-based generator.
//
//   token = argmax_v [ (x_v + mask_v - M) / T + g_v ],   g_v = -log(-log(u_v)),
//   u_v from word (v & 3) of Philox4x32-10 with key = seed and counter = (v >> 2, position, stream, attempt).
//
// The token is a pure function of the logits row and five integers: it does not depend on the launch shape, on which
// other rows share the batch or on how the row is dealt to the threads (the argmax is taken in the strict total order
// (key descending, id ascending) of every top-k of the engine).  One pass over the row, one block-wide reduction -- an
// inverse-CDF draw needs the normaliser of softmax(x / T) first (a second pass) and a prefix sum whose rounding depends on
// the block geometry.
//
//   dec_sample_update_kernel   behind the logits tail of a chained sampling step (decode_step.cpp): one block per row draws
//                              the row's token, records it with its untempered log-prob, and prepares the row for the next
//                              step (state words, position table, embedding row) -- dec_beam_update_kernel's work for
//                              independent rows.  Plain launch: no block waits for another block.
//   sample_rows_kernel         the draw alone on caller data (test hook wb_sample_rows): the same device function.
#include <hip/hip_runtime.h>

#include "decode.h"
#include "philox.h"
#include "wave_ops.h"

namespace wb {
namespace {

constexpr int SM_NT = 1024, SM_NW = SM_NT / 64;
constexpr int SM_PF = 4;             // Philox groups (4 ids each) per thread whose loads are requested together

struct SampleDraw { int id; int bad; };

// The draw of one row by one block of SM_NT threads (every thread of the block calls it; two barriers inside).
// x [V]: the row's logits; mask [V] or null; M: the row maximum under that mask.  Returns, in every thread, the winning id
// (0x7fffffff: no id had a finite key) and `bad` != 0 when a logit or a key of the row was NaN.
__device__ __forceinline__ SampleDraw sample_row_draw(const float* __restrict__ x, int V, const float* __restrict__ mask,
                                                      float M, float inv_t, uint32_t k0, uint32_t k1, uint32_t stream,
                                                      uint32_t attempt, uint32_t position, float* redv, int* redi,
                                                      int* redb) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = (V + 3) >> 2;
  float bv = -INFINITY;
  int bi = 0x7fffffff, bad = 0;
  for (int g0 = tid; g0 < G; g0 += SM_NT * SM_PF) {
    float xb[SM_PF][4], mb[SM_PF][4];
#pragma unroll
    for (int u = 0; u < SM_PF; u++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int c = 4 * (g0 + SM_NT * u) + q, cc = c < V ? c : 0;      // (past the row: re-read id 0, discarded below)
        xb[u][q] = x[cc];
        mb[u][q] = mask ? mask[cc] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < SM_PF; u++) {
      const int g = g0 + SM_NT * u;
      if (4 * g < V) {
        const U4 r = philox4x32_10((uint32_t)g, position, stream, attempt, k0, k1);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int c = 4 * g + q;
          if (c < V) {
            const float t = (xb[u][q] + mb[u][q]) - M;
            const float key = fmaf(t, inv_t, gumbel_of(r.w[q]));
            if (key != key) bad = 1;
            if (key > -INFINITY && better(key, c, bv, bi)) { bv = key; bi = c; }
          }
        }
      }
    }
  }
  wave_argmax(bv, bi);
  const int wbad = __ballot(bad) != 0ull ? 1 : 0;
  if (lane == 0) { redv[wave] = bv; redi[wave] = bi; redb[wave] = wbad; }
  __syncthreads();
  SampleDraw o;
  o.id = redi[0]; o.bad = redb[0];
  float gv = redv[0];
  for (int j = 1; j < SM_NW; j++) {
    if (better(redv[j], redi[j], gv, o.id)) { gv = redv[j]; o.id = redi[j]; }
    o.bad |= redb[j];
  }
  __syncthreads();                       // (the scratch words may be reused by the caller)
  return o;
}

__global__ __launch_bounds__(SM_NT) void dec_sample_update_kernel(SampleChainArgs a) {
  __shared__ float redv[SM_NW];
  __shared__ int redi[SM_NW], redb[SM_NW];
  const StepLayout& L = a.lay;
  const SampleChainLayout& B = a.sl;
  int* st = a.state;
  int* ctl = a.ctl;
  const int r = blockIdx.x, tid = threadIdx.x;
  // the row's words as they stand at kernel entry: every block reads and writes its own row only; ST_STEP belongs to block 0
  // and ST_N is written at most once per chain, by the block whose row finishes last (see dec_topk_merge_kernel)
  const int n_live = st[ST_N];
  if (r >= n_live || r >= B.S) return;
  const int len_now = st[L.len + r], tok_now = st[L.tok + r], w = st[L.win + r];
  const int fin_now = ctl[B.fin + r], ngen = ctl[B.ngen + r];
  int tok_next = tok_now, fin = fin_now;
  if (!fin_now && ngen < B.max_depth) {          // (block-uniform)
    const float M = a.row_stats[2 * r], lse = a.row_stats[2 * r + 1];
    const float* x = a.logits + (int64_t)r * a.V;
    const float* mk = a.use_mask ? a.mask : nullptr;
    const SampleDraw dr = sample_row_draw(x, a.V, mk, M, __int_as_float(ctl[SC_INVT]), (uint32_t)ctl[SC_SEED_LO],
                                          (uint32_t)ctl[SC_SEED_HI], (uint32_t)ctl[B.stream + r], (uint32_t)ctl[SC_ATTEMPT],
                                          (uint32_t)len_now, redv, redi, redb);
    // a row without a finite key or with a NaN logit ends on <|endoftext|> and fails the call: never an embedding index
    const bool bad = dr.bad != 0 || (unsigned)dr.id >= (unsigned)a.V;
    tok_next = bad ? a.eot : dr.id;
    fin = tok_next == a.eot ? 1 : 0;
    if (tid == 0) {
      double* sum = reinterpret_cast<double*>(ctl + B.sum);
      if (bad) ctl[SC_ERR] = 1;
      else sum[r] += (double)(((x[tok_next] + (mk ? mk[tok_next] : 0.f)) - M) - lse);   // log-softmax of the logits, not of logits / T
      ctl[B.tokens + r * B.max_depth + ngen] = tok_next;
      ctl[B.ngen + r] = ngen + 1;
      if (fin) {
        ctl[B.fin + r] = 1;
        // the window's last row: no block streams its cached K/V any more
        if (atomicAdd(&ctl[B.win_fin + w], 1) + 1 == ctl[SC_BEST_OF]) st[L.win_nb + w] = 0;
        if (atomicAdd(&ctl[SC_NDONE], 1) + 1 == ctl[SC_NROWS]) { ctl[SC_ALLDONE] = 1; st[ST_N] = 0; }
      }
    }
  }
  if (len_now >= a.Lmax) return;
  __syncthreads();                               // every thread has read the row's state words (a finished row takes no draw, so
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
  for (int p = tid; p < len_now; p += SM_NT) tab_new[r * a.Lmax + p] = tab_old[r * a.Lmax + p];
  if (tid == 0) tab_new[r * a.Lmax + len_now] = nstep * L.S + r;
  const float4* e = reinterpret_cast<const float4*>(a.E + (int64_t)tok_next * a.d);
  const float4* pp = reinterpret_cast<const float4*>(a.pos + (int64_t)len_now * a.d);
  float4* o = reinterpret_cast<float4*>(a.x + (int64_t)r * a.d);
  for (int c = tid; c < (a.d >> 2); c += SM_NT) {
    const float4 u = e[c], v = pp[c];
    o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}

__global__ __launch_bounds__(SM_NT) void sample_rows_kernel(SampleRowsArgs a) {
  __shared__ float redv[SM_NW];
  __shared__ int redi[SM_NW], redb[SM_NW];
  const int r = blockIdx.x;
  if (r >= a.R) return;
  const float M = a.row_stats[2 * r], lse = a.row_stats[2 * r + 1];
  const float* x = a.logits + (int64_t)r * a.ld;
  const float* mk = (a.mask && a.row_masked[r]) ? a.mask : nullptr;
  const SampleDraw dr = sample_row_draw(x, a.V, mk, M, a.inv_t, a.seed_lo, a.seed_hi, (uint32_t)a.stream[r], a.attempt,
                                        (uint32_t)a.position[r], redv, redi, redb);
  if (threadIdx.x == 0) {
    const bool bad = dr.bad != 0 || (unsigned)dr.id >= (unsigned)a.V;
    const int tok = bad ? a.eot : dr.id;
    if (bad) *a.out_err = 1;
    a.out_token[r] = tok;
    a.out_logprob[r] = bad ? 0.f : ((x[tok] + (mk ? mk[tok] : 0.f)) - M) - lse;
  }
}

}  // namespace

void launch_dec_sample_update(hipStream_t st, const SampleChainArgs& a, int n_rows) {
  WB_KLAUNCH(dec_sample_update_kernel, dim3(n_rows), dim3(SM_NT), 0, st, a);
}

void launch_sample_rows(hipStream_t st, const SampleRowsArgs& a) {
  WB_KLAUNCH(sample_rows_kernel, dim3(a.R), dim3(SM_NT), 0, st, a);
}

}  // namespace wb
