// Token scoring: log-softmax statistics of logits = h E^T without the logits.
//
//   score_logits_kernel   per (row tile, vocabulary split): 32 x 128 logits tiles on v_mfma_f32_32x32x2_f32 (exact f32, the
//                         arithmetic and LDS staging of gemm.hip's 32 x 128 configuration), each reduced ONLINE in registers
//                         to a per-row (max, sum exp(x - max)); the logit of the row's target and of the probe pairs is
//                         picked out of the tile that owns the column.  No logits tile reaches global memory.
//   score_merge_kernel    folds the splits' partials of a row in split order: lse, log-prob of the target, log-prob of
//                         the probes.
//
// Two statistics per row: its OWN (the additive mask applied when row_masked[r]) feeds lse / logprob; the UNMASKED one
// feeds the probes -- a row may be masked and carry probes (position 0 of a decoded row: the language token is scored under
// the special mask, the no-speech probability is not).  Without a masked row in the tile the two are one.
// Every result has exactly one writer and every fold a fixed order: no atomics, run-to-run bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace wb {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;
constexpr int BM = SCORE_BM, BN = SCORE_BN, BK = 32;
constexpr int LDA_S = BM + 4, LDB_S = BN + 4;
constexpr int KQ = BK / 4;                    // float4 quads per A row per k-tile
constexpr int B_F4 = (BK * BN / 4) / NT;      // float4 loads of B / thread / k-tile

// (max, sum) pairs: (-inf, 0) is the empty set; nothing here turns it into a NaN, and a NaN logit stays one (a NaN max
// poisons every later sum and every merge: the row's lse and log-probs come out NaN, not finite-looking)
__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
  if (x > m) { s = s * expf(m - x) + 1.f; m = x; }          // (m = -inf: s = 0 * 0 + 1)
  else if (x > -INFINITY) s += expf(x - m);                 // (x = -inf: a masked column, nothing to add; m NaN: s NaN)
  else if (x != x) { m = x; s = x; }
}
__device__ __forceinline__ float2 lse_merge(float2 a, float2 b) {
  if (a.x != a.x || b.x != b.x) return make_float2(a.x + b.x, a.x + b.x);   // (fmaxf would drop the NaN)
  const float M = fmaxf(a.x, b.x);
  if (M == -INFINITY) return make_float2(-INFINITY, 0.f);
  return make_float2(M, a.y * expf(a.x - M) + b.y * expf(b.x - M));
}

__global__ __launch_bounds__(NT, 2) void score_logits_kernel(ScoreArgs g) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDA_S];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB_S];
  __shared__ float Ts[BM][BN + 1];            // a logits tile, only when a probe column falls into it
  __shared__ int s_lo[NT], s_hi[NT], s_msk[BM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * BM, split = blockIdx.y;
  const int R = g.R, d = g.d, V = g.V, ldv = g.ldv;
  const int n_tiles = (V + BN - 1) / BN;
  const int t_beg = (int)((int64_t)split * n_tiles / g.vs), t_end = (int)((int64_t)(split + 1) * n_tiles / g.vs);

  // ---- block prologue: masked rows of the tile, column range of the tile's probes ----
  {
    int lo = 0x7fffffff, hi = -1;
    for (int p = tid; p < g.n_probe; p += NT) {
      const int r = g.probe_row[p] - m0;
      if (r >= 0 && r < BM) { const int id = g.probe_id[p]; lo = min(lo, id); hi = max(hi, id); }
    }
    s_lo[tid] = lo; s_hi[tid] = hi;
    if (tid < BM) s_msk[tid] = (g.mask && g.row_masked && m0 + tid < R && g.row_masked[m0 + tid]) ? 1 : 0;
  }
  __syncthreads();
  int pr_lo = 0x7fffffff, pr_hi = -1, any_masked = 0;
  for (int i = 0; i < NT; i++) { pr_lo = min(pr_lo, s_lo[i]); pr_hi = max(pr_hi, s_hi[i]); }
  for (int i = 0; i < BM; i++) any_masked |= s_msk[i];
  // this lane's 16 rows of a 32 x 32 accumulator: row(r) = 4 lh + (r & 3) + 8 (r >> 2)
  int tgt[16];
  unsigned mbits = 0;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int rl = 4 * lh + (r & 3) + 8 * (r >> 2);
    tgt[r] = (g.target && m0 + rl < R) ? g.target[m0 + rl] : -1;
    mbits |= (unsigned)s_msk[rl] << r;
  }
  float om[16], os[16], um[16], us[16];       // own / unmasked (max, sum) of this lane's columns
#pragma unroll
  for (int r = 0; r < 16; r++) { om[r] = um[r] = -INFINITY; os[r] = us[r] = 0.f; }

  const int a_r = tid / KQ, a_kq = (tid % KQ) * 4;
  const float* a_row = (m0 + a_r < R) ? g.h + (int64_t)(m0 + a_r) * d : nullptr;
  const int nk = d / BK;

  for (int t = t_beg; t < t_end; t++) {
    const int c0 = t * BN;
    float4 ra, rb[B_F4];
    auto load_tile = [&](int k0) {
      ra = a_row ? *reinterpret_cast<const float4*>(a_row + k0 + a_kq) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < B_F4; i++) {
        const int idx = tid + i * NT, kr = idx / (BN / 4), n = c0 + (idx % (BN / 4)) * 4;
        // columns [V, ldv) are read with their quad and never used; columns >= ldv do not exist
        rb[i] = n < ldv ? *reinterpret_cast<const float4*>(g.Et + (int64_t)(k0 + kr) * ldv + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto store_tile = [&](int buf) {
      As[buf][a_kq + 0][a_r] = ra.x; As[buf][a_kq + 1][a_r] = ra.y;
      As[buf][a_kq + 2][a_r] = ra.z; As[buf][a_kq + 3][a_r] = ra.w;
#pragma unroll
      for (int i = 0; i < B_F4; i++) {
        const int idx = tid + i * NT, kr = idx / (BN / 4), n4 = (idx % (BN / 4)) * 4;
        *reinterpret_cast<float4*>(&Bs[buf][kr][n4]) = rb[i];
      }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    load_tile(0);
    store_tile(0);
    if (nk > 1) load_tile(BK);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
      const int buf = kt & 1;
#pragma unroll
      for (int kk = 0; kk < BK / 2; kk++) {
        const int kidx = 2 * kk + lh;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[buf][kidx][li], Bs[buf][kidx][wave * 32 + li], acc, 0, 0, 0);
      }
      if (kt + 1 < nk) {
        store_tile(buf ^ 1);
        if (kt + 2 < nk) load_tile((kt + 2) * BK);
      }
      __syncthreads();
    }
    // ---- the tile's epilogue: online (max, sum), target pick; columns [V, ..) contribute nothing ----
    const int col = c0 + wave * 32 + li;
    if (col < V) {
      const float mk = any_masked ? g.mask[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const float x = acc[r];
        const float xo = ((mbits >> r) & 1u) ? x + mk : x;
        lse_push(om[r], os[r], xo);
        if (any_masked) lse_push(um[r], us[r], x);
        if (col == tgt[r]) g.target_logit[m0 + 4 * lh + (r & 3) + 8 * (r >> 2)] = xo;
      }
    }
    if (pr_hi >= c0 && pr_lo < c0 + BN) {     // (block-uniform) probe logits, unmasked, out of the tile in LDS
#pragma unroll
      for (int r = 0; r < 16; r++) Ts[4 * lh + (r & 3) + 8 * (r >> 2)][wave * 32 + li] = acc[r];
      __syncthreads();
      for (int p = tid; p < g.n_probe; p += NT) {
        const int r = g.probe_row[p] - m0, c = g.probe_id[p] - c0;
        if (r >= 0 && r < BM && c >= 0 && c < BN) g.probe_logit[p] = Ts[r][c];
      }
      // (the next write of Ts is behind the next tile's k loop: at least one barrier)
    }
  }

  // ---- fold the 128 column slots of every row, fixed order: 8 segments of 16, then the 8 ----
  float2* red = reinterpret_cast<float2*>(&Bs[0][0][0]);      // [BM][BN]   (the k loops are over: see the last barrier)
  float2* red2 = reinterpret_cast<float2*>(&As[0][0][0]);     // [BM][8]
  static_assert(sizeof(Bs) >= BM * BN * sizeof(float2) && sizeof(As) >= BM * 8 * sizeof(float2), "reduction scratch");
  float2 res[2];
  for (int stat = 0; stat < (any_masked ? 2 : 1); stat++) {
#pragma unroll
    for (int r = 0; r < 16; r++)
      red[(4 * lh + (r & 3) + 8 * (r >> 2)) * BN + wave * 32 + li] =
          stat == 0 ? make_float2(om[r], os[r]) : make_float2(um[r], us[r]);
    __syncthreads();
    {
      const int row = tid >> 3, seg = tid & 7;
      float2 a = red[row * BN + seg * 16];
      for (int i = 1; i < 16; i++) a = lse_merge(a, red[row * BN + seg * 16 + i]);
      red2[row * 8 + seg] = a;
    }
    __syncthreads();
    if (tid < BM) {
      float2 a = red2[tid * 8];
      for (int i = 1; i < 8; i++) a = lse_merge(a, red2[tid * 8 + i]);
      res[stat] = a;
    }
    __syncthreads();
  }
  if (tid < BM && m0 + tid < R) {
    const float2 o = res[0], u = any_masked ? res[1] : res[0];
    g.part[(int64_t)split * R + m0 + tid] = make_float4(o.x, o.y, u.x, u.y);
  }
}

__global__ __launch_bounds__(NT) void score_merge_kernel(ScoreArgs g) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= g.R + g.n_probe) return;
  const bool probe = idx >= g.R;
  const int row = probe ? g.probe_row[idx - g.R] : idx;
  float2 a = make_float2(-INFINITY, 0.f);
  for (int s = 0; s < g.vs; s++) {            // split order
    const float4 p = g.part[(int64_t)s * g.R + row];
    a = lse_merge(a, probe ? make_float2(p.z, p.w) : make_float2(p.x, p.y));
  }
  const float lse = a.x == -INFINITY ? -INFINITY : a.x + logf(a.y);
  if (probe) {
    g.probe_lp[idx - g.R] = g.probe_logit[idx - g.R] - lse;
  } else {
    g.lse[row] = lse;
    g.logprob[row] = (g.target && g.target[row] >= 0) ? g.target_logit[row] - lse : __int_as_float(0x7fc00000);
  }
}

}  // namespace

int score_splits(int R, int V, int requested) {
  const int n_tiles = (V + BN - 1) / BN, row_tiles = (R + BM - 1) / BM;
  // auto: about two blocks per CU (59 KB of LDS each) whatever R is -- language detection scores one row per window
  int vs = requested > 0 ? requested : (512 + row_tiles - 1) / row_tiles;
  return std::max(1, std::min(vs, n_tiles));
}

int launch_score_logits(hipStream_t st, const ScoreArgs& a) {
  if (a.R <= 0 || a.V <= 0 || a.d < BK || a.d % BK != 0 || a.ldv % 4 != 0 || a.ldv < a.V) return -1;
  if (a.vs < 1 || a.vs > (a.V + BN - 1) / BN || a.n_probe < 0) return -1;
  WB_KLAUNCH(score_logits_kernel, dim3((a.R + BM - 1) / BM, a.vs), dim3(NT), 0, st, a);
  return 0;
}

void launch_score_merge(hipStream_t st, const ScoreArgs& a) {
  WB_KLAUNCH(score_merge_kernel, dim3((a.R + a.n_probe + NT - 1) / NT), dim3(NT), 0, st, a);
}

}  // namespace wb
