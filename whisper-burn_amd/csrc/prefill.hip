// Prompt prefill: the way from the teacher-forced pass's qkv planes (engine.cpp: decoder_blocks) into the paged self-KV
// cache and the position tables the step kernels read.  HBM-bound copies; plain launches ordered by the stream.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace wb {
namespace {

// One block per pass row r = a * n + p (active window a, prompt position p): columns [d, 2d) and [2d, 3d) of qkv row r go
// to row p * S + a of Kc / Vc -- dec_prepare_kernel's tabs[...] = step * S + slot with step = p, slot = a.  K arrives
// pre-scaled by the QKV GEMM's col_scale and V with its bias, as dec_self_attn_kernel stores them.  16 B per lane, consecutive
// lanes along d: a wave moves 1 KiB of one row per instruction.  tabs non-null (the first layer's launch): the block also
// writes its entry of the table parity that step n reads as tab_old.  Nothing else is touched.
__global__ __launch_bounds__(128) void prefill_store_kernel(const float* __restrict__ qkv, int n, int d, int ld, int S, int Lmax,
                                                            float* __restrict__ Kc, float* __restrict__ Vc,
                                                            int* __restrict__ tabs) {
  const int r = blockIdx.x;
  const int a = r / n, p = r - a * n;
  const int64_t row = (int64_t)p * S + a;
  const int d4 = d >> 2;
  const float4* src = reinterpret_cast<const float4*>(qkv + (int64_t)r * ld + d);   // K | V: 2 d contiguous floats
  float4* kd = reinterpret_cast<float4*>(Kc + row * d);
  float4* vd = reinterpret_cast<float4*>(Vc + row * d);
  for (int c = threadIdx.x; c < 2 * d4; c += blockDim.x) {
    const float4 v = src[c];
    if (c < d4) kd[c] = v;
    else vd[c - d4] = v;
  }
  if (tabs && threadIdx.x == 0) tabs[(int64_t)((n - 1) & 1) * S * Lmax + (int64_t)a * Lmax + p] = (int)row;
}

}  // namespace

int launch_prefill_store(hipStream_t st, const float* qkv, int nA, int n, int d, int ld, int S, int Lmax, float* Kc, float* Vc,
                         int* tabs) {
  // (16-byte accesses: d and ld in floats are multiples of 4; the caller's bases are allocation-aligned)
  if (nA < 1 || n < 1 || nA > S || n > Lmax || d < 4 || d % 4 != 0 || ld % 4 != 0 || ld < 3 * d) return -1;
  if ((int64_t)nA * n >= ((int64_t)1 << 31) || (int64_t)Lmax * S >= ((int64_t)1 << 31)) return -1;
  WB_KLAUNCH(prefill_store_kernel, dim3(nA * n), dim3(128), 0, st, qkv, n, d, ld, S, Lmax, Kc, Vc, tabs);
  return 0;
}

}  // namespace wb
