// Token alignment: cross-attention weights that are KEPT, their normalise / median / head-mean stage, and DTW on the device.
//
// The decode kernels are flash-style and never hold an attention weight.  Alignment needs the weights of a few heads over
// the finished token row -- softmax_c((q_l s) . (k_c s)) for every token l and encoder position c -- but only long enough
// to fold them into ONE [len][C] matrix per row: z-score down the token axis, median filter along c, mean over the heads.
// Three kernels, all exact f32 (the result feeds a discrete decision: no split precision, no fast exp):
//
//   align_row_stats   (max, sum) of every score row, per (head, row, token): two passes over the keys on
//                     v_mfma_f32_32x32x2_f32 -- the exact maximum first, then sum exp(s - max) with no rescaling.
//   align_accumulate  per (row, strip of encoder positions + halo): for each head of the layer, in the order given,
//                     recompute the strip's scores (the same MFMA chain: bit-identical to the first kernel's), normalise,
//                     keep [len][64] in LDS, z-score every column, median along the strip, add into M.  One block owns
//                     its elements of M and walks the heads in order: no atomics, run-to-run bit-identical.
//   align_dtw         one block per row, a thread per token, anti-diagonal wavefront; the only arithmetic is one f32 add
//                     per cell and strict comparisons (bit-reproducible against the NumPy f32 recurrence); the trace is one
//                     byte per cell in global memory, the backtrace runs on the device.
//
// MFMA operand layout as in attention.hip ("swapped": S^T[kv][q] = K_tile Q^T): lane (j, h) supplies K[kv0 + j][32 h + s]
// and Q[q0 + j][32 h + s] at step s and owns S^T[(r & 3) + 8 (r >> 2) + 4 h][j] in accumulator register r.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "wave_ops.h"

namespace wb {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void load32(const float* p, float (&r)[32]) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float4 v = p4[i];
    r[4 * i + 0] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
  }
}

// one 32-key x 32-query tile of scores; Q and K arrive pre-scaled (the GEMMs that made them applied dh^-0.25)
__device__ __forceinline__ f32x16 score_tile(const float (&kreg)[32], const float (&qreg)[32]) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 32; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[s], qreg[s], acc, 0, 0, 0);
  return acc;
}

// grid (q blocks of 32, heads of the layer, rows), one wave per block
__global__ __launch_bounds__(64) void align_row_stats_kernel(const float* __restrict__ Q, int ldq,
                                                             const float* __restrict__ K, int ldkv,
                                                             const AttnSeg* __restrict__ segs,
                                                             const int32_t* __restrict__ heads,
                                                             float2* __restrict__ stats, int ld_stats) {
  const AttnSeg seg = segs[blockIdx.z];
  const int q0 = blockIdx.x * 32;
  if (q0 >= seg.q_len) return;
  const int head = heads[blockIdx.y];
  const int lane = threadIdx.x, li = lane & 31, hh = lane >> 5;
  const int qi = q0 + li;
  float qreg[32], kreg[32];
  load32(Q + (int64_t)(seg.q_row0 + min(qi, seg.q_len - 1)) * ldq + head * 64 + hh * 32, qreg);
  const float* Kb = K + (int64_t)seg.kv_row0 * ldkv + head * 64 + hh * 32;
  const int n_tiles = (seg.kv_len + 31) / 32;
  float m = -INFINITY;
  for (int t = 0; t < n_tiles; t++) {
    load32(Kb + (int64_t)min(t * 32 + li, seg.kv_len - 1) * ldkv, kreg);
    const f32x16 s = score_tile(kreg, qreg);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int kv = t * 32 + 4 * hh + (r & 3) + 8 * (r >> 2);
      if (kv < seg.kv_len) m = fmaxf(m, s[r]);
    }
  }
  m = xor32_max(m);
  float l = 0.f;
  for (int t = 0; t < n_tiles; t++) {
    load32(Kb + (int64_t)min(t * 32 + li, seg.kv_len - 1) * ldkv, kreg);
    const f32x16 s = score_tile(kreg, qreg);
    float psum = 0.f;       // the tile's own short chain, then one add into the running sum
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int kv = t * 32 + 4 * hh + (r & 3) + 8 * (r >> 2);
      if (kv < seg.kv_len) psum += expf(s[r] - m);
    }
    l += psum;
  }
  l = xor32_sum(l);
  if (qi < seg.q_len && hh == 0)
    stats[((int64_t)blockIdx.y * gridDim.z + blockIdx.z) * ld_stats + qi] = make_float2(m, l);
}

constexpr int ACC_TILE = 64;        // encoder positions per block, halo included (two MFMA key tiles)
constexpr int ACC_LD = ACC_TILE + 1;
constexpr int ACC_THREADS = 256;

// median of FW values (FW odd): partial selection sort up to the middle element
template <int FW>
__device__ __forceinline__ float median_of(float (&v)[FW]) {
#pragma unroll
  for (int i = 0; i <= FW / 2; i++)
#pragma unroll
    for (int j = i + 1; j < FW; j++) {
      const float a = v[i], b = v[j];
      v[i] = fminf(a, b); v[j] = fmaxf(a, b);
    }
  return v[FW / 2];
}

// grid (strips, rows), ACC_THREADS threads, dynamic LDS: max_len * ACC_LD floats.
// first != 0: this launch holds the first head of the whole list (M is written, not added to);
// n_total > 0: it holds the last one (M becomes sum / n_total).
template <int FW>
__global__ __launch_bounds__(ACC_THREADS) void align_accumulate_kernel(const float* __restrict__ Q, int ldq,
                                                                       const float* __restrict__ K, int ldkv,
                                                                       const AttnSeg* __restrict__ segs,
                                                                       const int32_t* __restrict__ heads, int n_heads,
                                                                       const float2* __restrict__ stats, int ld_stats,
                                                                       float* __restrict__ M, int ld_row, int ldm,
                                                                       int first, int n_total) {
  HIP_DYNAMIC_SHARED(float, Wt)                       // [q_len][ACC_LD]: weights, then z-scores, of one head
  __shared__ float part[4][ACC_TILE];
  __shared__ float part2[4][ACC_TILE];
  constexpr int HW = FW / 2, SU = ACC_TILE - 2 * HW;  // halo, useful positions per strip
  const AttnSeg seg = segs[blockIdx.y];
  const int C = seg.kv_len, len = seg.q_len;
  const int c_out0 = blockIdx.x * SU;                 // first position this block writes
  if (c_out0 >= C || len <= 0) return;
  const int c_begin = c_out0 - HW;                    // position of LDS column 0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, hh = lane >> 5;
  const bool filter = C > HW;                         // a window shorter than the halo is not filtered
  const int n_qb = (len + 31) / 32;
  const int n_rows = gridDim.y;
  float* Mrow = M + (int64_t)blockIdx.y * ld_row * ldm;

  for (int hi = 0; hi < n_heads; hi++) {
    const int head = heads[hi];
    // ---- weights of the strip: W[q][c] = exp(s - max_q) / sum_q ----
    {
      float k0[32], k1[32], qreg[32];
      const float* Kb = K + (int64_t)seg.kv_row0 * ldkv + head * 64 + hh * 32;
      load32(Kb + (int64_t)min(max(c_begin + li, 0), C - 1) * ldkv, k0);
      load32(Kb + (int64_t)min(max(c_begin + 32 + li, 0), C - 1) * ldkv, k1);
      const float2* st = stats + ((int64_t)hi * n_rows + blockIdx.y) * ld_stats;
      for (int qb = wave; qb < n_qb; qb += ACC_THREADS / 64) {
        const int qi = qb * 32 + li, qrow = min(qi, len - 1);
        load32(Q + (int64_t)(seg.q_row0 + qrow) * ldq + head * 64 + hh * 32, qreg);
        const float2 ml = st[qrow];
#pragma unroll
        for (int t = 0; t < 2; t++) {
          const f32x16 s = score_tile(t == 0 ? k0 : k1, qreg);
          if (qi < len) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const int col = t * 32 + 4 * hh + (r & 3) + 8 * (r >> 2), c = c_begin + col;
              Wt[qi * ACC_LD + col] = (c >= 0 && c < C) ? expf(s[r] - ml.x) / ml.y : 0.f;
            }
          }
        }
      }
    }
    __syncthreads();
    // ---- z-score down the token axis, per column: biased variance, a constant column gives zeros ----
    {
      const int col = tid & (ACC_TILE - 1), p = tid >> 6;
      float s = 0.f;
      for (int q = p; q < len; q += 4) s += Wt[q * ACC_LD + col];
      part[p][col] = s;
      __syncthreads();
      const float mean = ((part[0][col] + part[1][col]) + (part[2][col] + part[3][col])) / (float)len;
      float s2 = 0.f;
      for (int q = p; q < len; q += 4) { const float dlt = Wt[q * ACC_LD + col] - mean; s2 += dlt * dlt; }
      part2[p][col] = s2;
      __syncthreads();
      const float sd = sqrtf(((part2[0][col] + part2[1][col]) + (part2[2][col] + part2[3][col])) / (float)len);
      for (int q = p; q < len; q += 4) {
        const float w = Wt[q * ACC_LD + col];
        Wt[q * ACC_LD + col] = sd > 0.f ? (w - mean) / sd : 0.f;
      }
    }
    __syncthreads();
    // ---- median along the strip (reflect padding: c = -1 -> 1), added into M ----
    const bool is_first = first && hi == 0, is_last = n_total > 0 && hi == n_heads - 1;
    for (int idx = tid; idx < len * SU; idx += ACC_THREADS) {
      const int q = idx / SU, c = c_out0 + idx % SU;
      if (c >= C) continue;
      float med;
      if (filter) {
        float v[FW];
#pragma unroll
        for (int k = 0; k < FW; k++) {
          int cc = c + k - HW;
          cc = cc < 0 ? -cc : cc;
          cc = cc >= C ? 2 * (C - 1) - cc : cc;
          v[k] = Wt[q * ACC_LD + (cc - c_begin)];
        }
        med = median_of<FW>(v);
      } else {
        med = Wt[q * ACC_LD + (c - c_begin)];
      }
      float* mp = Mrow + (int64_t)q * ldm + c;
      float acc = is_first ? med : *mp + med;
      if (is_last) acc = acc / (float)n_total;
      *mp = acc;
    }
    __syncthreads();
  }
}

constexpr int DTW_MAX_N = 512;

// grid (rows), block = max N rounded up to a wave.  Thread i owns DTW row i; on anti-diagonal d it computes cell (i, d - i)
// from its own last value (left), its upper neighbour's last value (up, through LDS) and the value it read from that
// neighbour one diagonal earlier (diagonal).  Trace codes 0 / 1 / 2 = diagonal / up / left, four cells per stored word.
__global__ __launch_bounds__(DTW_MAX_N) void align_dtw_kernel(const float* __restrict__ X, int ldx, int negate,
                                                              const DtwSeg* __restrict__ segs,
                                                              uint32_t* __restrict__ trace, int64_t trace_stride, int ldt,
                                                              int32_t* __restrict__ out) {
  __shared__ float last[2][DTW_MAX_N + 1];            // [diagonal parity][thread + 1]; entry 0: the border row (+inf)
  const DtwSeg seg = segs[blockIdx.x];
  const int N = seg.n, C = seg.c, i = threadIdx.x;
  if (N <= 0 || C <= 0) return;
  uint32_t* tr = trace + (int64_t)blockIdx.x * trace_stride;
  for (int k = i; k < 2 * (DTW_MAX_N + 1); k += blockDim.x) (&last[0][0])[k] = INFINITY;
  __syncthreads();
  const float* xr = X + (int64_t)(seg.x_row0 + i) * ldx;
  float left = INFINITY, diag = i == 0 ? 0.f : INFINITY;
  uint32_t pack = 0;
  const int n_diag = N + C - 1;
  for (int d = 0; d < n_diag; d++) {
    const int j = d - i;
    if (i < N && j >= 0 && j < C) {
      const float up = last[(d + 1) & 1][i];
      const float x = negate ? -xr[j] : xr[j];
      float c;
      uint32_t t;
      if (diag < up && diag < left) { c = diag; t = 0; }
      else if (up < diag && up < left) { c = up; t = 1; }
      else { c = left; t = 2; }
      const float cost = x + c;
      pack |= t << (8 * (j & 3));
      if ((j & 3) == 3 || j == C - 1) { tr[(int64_t)i * ldt + (j >> 2)] = pack; pack = 0; }
      last[d & 1][i + 1] = cost;
      left = cost;
      diag = up;
    }
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  if (i == 0) {      // backtrace from (N - 1, C - 1); the first row only moves left, the first column only up
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(tr);
    int r = N - 1, j = C - 1;
    while (r > 0 || j > 0) {
      int t = tb[((int64_t)r * ldt) * 4 + j];
      if (r == 0) t = 2;
      else if (j == 0) t = 1;
      if (t == 2) { j--; continue; }
      out[seg.out0 + r] = j;                          // leaving row r: j is the row's first path cell
      r--;
      if (t == 0) j--;
    }
    out[seg.out0] = 0;
  }
}

}  // namespace

void launch_align_row_stats(hipStream_t st, const float* Q, int ldq, const float* K, int ldkv, const AttnSeg* segs_dev,
                            int n_rows, int max_len, const int32_t* heads_dev, int n_heads, float2* stats, int ld_stats) {
  if (n_rows <= 0 || n_heads <= 0 || max_len <= 0) return;
  WB_KLAUNCH(align_row_stats_kernel, dim3((max_len + 31) / 32, n_heads, n_rows), dim3(64), 0, st, Q, ldq, K, ldkv, segs_dev,
             heads_dev, stats, ld_stats);
}

template <int FW>
static int launch_accumulate_fw(hipStream_t st, const float* Q, int ldq, const float* K, int ldkv, const AttnSeg* segs_dev,
                                int n_rows, int max_len, int max_C, const int32_t* heads_dev, int n_heads,
                                const float2* stats, int ld_stats, float* M, int ld_row, int ldm, int first, int n_total) {
  const size_t lds = (size_t)max_len * ACC_LD * sizeof(float);
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)align_accumulate_kernel<FW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess)
    return -1;
  const int su = ACC_TILE - 2 * (FW / 2);
  WB_KLAUNCH(align_accumulate_kernel<FW>, dim3((max_C + su - 1) / su, n_rows), dim3(ACC_THREADS), lds, st, Q, ldq, K, ldkv,
             segs_dev, heads_dev, n_heads, stats, ld_stats, M, ld_row, ldm, first, n_total);
  return 0;
}

int launch_align_accumulate(hipStream_t st, const float* Q, int ldq, const float* K, int ldkv, const AttnSeg* segs_dev,
                            int n_rows, int max_len, int max_C, const int32_t* heads_dev, int n_heads, const float2* stats,
                            int ld_stats, float* M, int ld_row, int ldm, int filter_width, int first, int n_total) {
  if (n_rows <= 0 || n_heads <= 0 || max_len <= 0 || max_C <= 0) return -1;
  if (max_len > ALIGN_MAX_LEN) return -1;
#define WB_ACC(FW)                                                                                                     \
  case FW:                                                                                                             \
    return launch_accumulate_fw<FW>(st, Q, ldq, K, ldkv, segs_dev, n_rows, max_len, max_C, heads_dev, n_heads, stats,  \
                                    ld_stats, M, ld_row, ldm, first, n_total);
  switch (filter_width) {
    WB_ACC(1) WB_ACC(3) WB_ACC(5) WB_ACC(7) WB_ACC(9) WB_ACC(11) WB_ACC(13) WB_ACC(15)
    default: return -1;
  }
#undef WB_ACC
}

int launch_align_dtw(hipStream_t st, const float* X, int ldx, int negate, const DtwSeg* segs_dev, int n_rows, int max_n,
                     uint32_t* trace, int64_t trace_stride, int ldt, int32_t* out) {
  if (n_rows <= 0 || max_n <= 0 || max_n > DTW_MAX_N) return -1;
  WB_KLAUNCH(align_dtw_kernel, dim3(n_rows), dim3((max_n + 63) / 64 * 64), 0, st, X, ldx, negate, segs_dev, trace,
             trace_stride, ldt, out);
  return 0;
}

}  // namespace wb
