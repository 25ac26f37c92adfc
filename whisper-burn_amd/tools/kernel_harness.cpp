// Test-only harness around the host-callable kernel launchers (csrc/kernels.h, csrc/decode.h): lib/libwhisper_hip_ktest.so.
// NOT part of the product ABI (include/whisper_hip.h does not know it); tests/test_gpu_kernels.py and
// tests/test_kernel_harness_emu.py drive it through ctypes.
//
// Every entry point takes HOST arrays, copies each one verbatim into a device allocation of the same size, calls ONE wb::launch_*
// function of the already-built library, synchronises, and copies the output arrays back.  It contains no kernel.  The caller
// hands in arrays that are LARGER than the contract (guard bands, padded leading dimensions, poisoned padding) together with the
// byte offset at which the launcher's pointer starts inside the array; the harness verifies -- before any launch -- that
// everything the contract lets the kernel touch lies inside those arrays and honours the alignment contracts of kernels.h.
// A wrong kernel therefore shows up as a failed comparison in the test, not as a memory fault.
//
// Return value: the launcher's own status (0 / -1; void launchers: 0), WBK_EARG when the arguments fail the harness's checks
// (nothing was launched), or -(1000 + hipError_t) for a HIP error.  Never aborts.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "decode.h"
#include "kernels.h"

namespace {

constexpr int WBK_EARG = -2;

struct Pool {                       // the device copies of one call
  std::vector<void*> dev;
  int err = 0;                      // first HIP error, as -(1000 + code)
  ~Pool() { for (void* p : dev) (void)hipFree(p); }
  bool ok(hipError_t e) { if (e != hipSuccess && err == 0) err = -(1000 + (int)e); return e == hipSuccess; }
};

extern "C" {
// one host array: `bytes` long, the launcher's pointer starts `off` bytes into its device copy.  host == null: null pointer.
struct WbkBuf { void* host; int64_t bytes; int64_t off; };
}

// device copy of b (verbatim); returns the base of the copy or null
char* upload(Pool& P, const WbkBuf& b) {
  if (!b.host || b.bytes <= 0) return nullptr;
  void* d = nullptr;
  if (!P.ok(hipMalloc(&d, (size_t)b.bytes))) return nullptr;
  P.dev.push_back(d);
  P.ok(hipMemcpy(d, b.host, (size_t)b.bytes, hipMemcpyHostToDevice));
  return (char*)d;
}
void download(Pool& P, const WbkBuf& b, const char* d) {
  if (d && b.host) P.ok(hipMemcpy(b.host, d, (size_t)b.bytes, hipMemcpyDeviceToHost));
}
// [lo, hi) in ELEMENTS of size esz relative to the launcher's pointer: inside the array?
bool inside(const WbkBuf& b, int64_t lo, int64_t hi, int esz) {
  if (!b.host) return false;
  const int64_t blo = b.off + lo * esz, bhi = b.off + hi * esz;
  return lo <= hi && blo >= 0 && bhi <= b.bytes;
}
bool aligned16(const WbkBuf& b, int64_t elem, int esz) { return ((b.off + elem * esz) & 15) == 0; }
int finish(Pool& P, int status) {
  P.ok(hipGetLastError());
  P.ok(hipStreamSynchronize(nullptr));
  return P.err ? P.err : status;
}

}  // namespace

extern "C" {

struct WbkGemm {
  int64_t variant;                  // 0: launch_gemm_f32, 1: launch_gemm_f16x3 (weight split on the device from W)
  WbkBuf A, Ah, Al, desc, B, W, Wh, Wl, C, Ch, Cl, bias, residual, aux, aux_idx;
  int64_t residual_is_c;            // 1: residual = the C pointer itself (the aliasing the contract allows)
  int64_t lda, a_mask_align, conv1_tstride, ldb, ldc, ldr, ld_aux, n_aux_rows;
  int64_t col_scale_period, col_scale_width, M, N, K, act, ksplit, c_split_stride, c_block_cols, c_block_stride, ldwt;
  int64_t use_range_flag, range_flag_out;
  double col_scale;
};

// A, B, bias, residual, aux, aux_idx, desc, W: inputs.  C (or Ch / Cl), Wh / Wl: copied in AND back.
int wbk_gemm(WbkGemm* g) {
  const int64_t M = g->M, N = g->N, K = g->K;
  if (M < 1 || N < 1 || K < 0 || M > (1 << 20) || N > (1 << 20) || K > (1 << 20)) return WBK_EARG;
  const bool f16 = g->variant == 1, pre = g->Ah.host != nullptr, pieces_out = g->Ch.host != nullptr;
  const bool conv1 = g->conv1_tstride > 0;
  const int64_t Kc = (K + 31) / 32 * 32;                       // a refused K never reaches a kernel; the checks use the padded one
  // ---- A ----
  const wb::RowDesc* hd = (const wb::RowDesc*)g->desc.host;
  if (hd && (g->desc.off != 0 || g->desc.bytes < M * (int64_t)sizeof(wb::RowDesc))) return WBK_EARG;
  if (conv1) {
    if (!hd || K % 3 != 0 || pre) return WBK_EARG;
    for (int64_t m = 0; m < M; m++) {
      const int64_t lo = hd[m].off - 1 + (hd[m].klo ? 1 : 0), hi = hd[m].off + (K / 3 - 1) * g->conv1_tstride + 2 - (hd[m].khi ? 1 : 0);
      if (!inside(g->A, lo, hi, 4)) return WBK_EARG;
    }
  } else if (pre) {
    if (!f16) return WBK_EARG;
    // (Ah without Al is one of the launcher's own refusals: it returns before any launch, so Al's extent is moot)
    if (g->Al.host && (g->Al.bytes != g->Ah.bytes || g->Al.off != g->Ah.off)) return WBK_EARG;
    if (!inside(g->Ah, 0, (M - 1) * g->lda + Kc, 2) || (g->lda % 8 == 0 && !aligned16(g->Ah, 0, 2))) return WBK_EARG;
  } else {
    for (int64_t m = 0; m < M; m++) {
      const int64_t start = hd ? hd[m].off : m * g->lda;
      int64_t klo = hd ? hd[m].klo : 0, khi = hd ? hd[m].khi : Kc;
      if (klo < 0 || khi > Kc) return WBK_EARG;
      if (hd && (klo % g->a_mask_align || khi % g->a_mask_align || g->a_mask_align < 1)) return WBK_EARG;
      if (f16 && hd && g->a_mask_align % 8 != 0) return WBK_EARG;   // the split kernel stages whole octets (kernels.h)
      if (!aligned16(g->A, start, 4)) return WBK_EARG;              // rows are read as float4
      if (khi > klo && !inside(g->A, start + klo / 4 * 4, start + (khi + 3) / 4 * 4, 4)) return WBK_EARG;
    }
  }
  // ---- B / W ----
  if (!f16) {
    if (g->ldb % 4 == 0 && (!inside(g->B, 0, Kc * g->ldb, 4) || !aligned16(g->B, 0, 4) || g->ldb < N)) return WBK_EARG;
  } else {
    if (g->W.off != 0 || g->W.bytes != K * N * 4 || g->Wh.off != 0 || g->Wl.off != 0) return WBK_EARG;
    if (g->ldwt < K || g->Wh.bytes != g->Wl.bytes || g->Wh.bytes < ((N - 1) * g->ldwt + Kc) * 2 || !g->Wh.host || !g->Wl.host)
      return WBK_EARG;
    if (g->ldwt != K && g->ldwt % 8 == 0) return WBK_EARG;     // launch_split_weight_f16 writes dense [N][K] rows
  }
  // ---- C ----
  const int64_t nsplit = g->ksplit > 1 ? g->ksplit : 1;
  const int64_t ncb = g->c_block_cols > 0 ? (N + g->c_block_cols - 1) / g->c_block_cols : 1;
  const int64_t cw = g->c_block_cols > 0 ? std::min<int64_t>(g->c_block_cols, N) : N;
  if (g->c_split_stride < 0 || g->c_block_stride < 0 || g->ldc < cw) return WBK_EARG;
  const int64_t c_hi = (nsplit - 1) * g->c_split_stride + (ncb - 1) * g->c_block_stride + (M - 1) * g->ldc + cw;
  if (pieces_out) {
    if (!f16) return WBK_EARG;                                   // only the split-precision kernel knows piece outputs
    if (!g->Cl.host || g->Cl.bytes != g->Ch.bytes || g->Cl.off != g->Ch.off || !inside(g->Ch, 0, c_hi, 2)) return WBK_EARG;
  } else if (!inside(g->C, 0, c_hi, 4)) {
    return WBK_EARG;
  }
  // ---- epilogue operands ----
  if (g->bias.host && !inside(g->bias, 0, N, 4)) return WBK_EARG;
  if (g->residual_is_c && (pieces_out || g->residual.host)) return WBK_EARG;
  if (g->residual.host && !inside(g->residual, 0, (M - 1) * g->ldr + N, 4)) return WBK_EARG;
  if (g->aux.host) {
    const int32_t* ix = (const int32_t*)g->aux_idx.host;
    if (!ix || g->aux_idx.off != 0 || g->aux_idx.bytes < M * 4 || g->n_aux_rows < 1) return WBK_EARG;
    for (int64_t m = 0; m < M; m++) if (ix[m] < 0 || ix[m] >= g->n_aux_rows) return WBK_EARG;
    if (!inside(g->aux, 0, (g->n_aux_rows - 1) * g->ld_aux + N, 4)) return WBK_EARG;
  }

  Pool P;
  char *dA = upload(P, g->A), *dAh = upload(P, g->Ah), *dAl = upload(P, g->Al), *dD = upload(P, g->desc), *dB = upload(P, g->B);
  char *dW = upload(P, g->W), *dWh = upload(P, g->Wh), *dWl = upload(P, g->Wl), *dC = upload(P, g->C), *dCh = upload(P, g->Ch);
  char *dCl = upload(P, g->Cl), *dbias = upload(P, g->bias), *dres = upload(P, g->residual), *daux = upload(P, g->aux);
  char* dix = upload(P, g->aux_idx);
  int* dflag = nullptr;
  if (g->use_range_flag) {
    void* p = nullptr;
    if (P.ok(hipMalloc(&p, 4))) { P.dev.push_back(p); P.ok(hipMemset(p, 0, 4)); dflag = (int*)p; }
  }
  if (P.err) return P.err;
  auto at = [](char* d, const WbkBuf& b) -> char* { return d ? d + b.off : nullptr; };

  wb::GemmArgs a;
  a.A = (const float*)at(dA, g->A); a.lda = g->lda;
  a.a_desc = (const wb::RowDesc*)dD; a.a_mask_align = (int)g->a_mask_align; a.conv1_tstride = (int)g->conv1_tstride;
  a.B = (const float*)at(dB, g->B); a.ldb = (int)g->ldb;
  a.C = (float*)at(dC, g->C); a.ldc = (int)g->ldc;
  a.bias = (const float*)at(dbias, g->bias);
  a.residual = g->residual_is_c ? a.C : (const float*)at(dres, g->residual); a.ldr = (int)g->ldr;
  a.aux = (const float*)at(daux, g->aux); a.aux_idx = (const int32_t*)dix; a.ld_aux = (int)g->ld_aux;
  a.col_scale = (float)g->col_scale; a.col_scale_period = (int)g->col_scale_period; a.col_scale_width = (int)g->col_scale_width;
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.act = (int)g->act;
  a.ksplit = (int)g->ksplit; a.c_split_stride = g->c_split_stride;
  a.c_block_cols = (int)g->c_block_cols; a.c_block_stride = g->c_block_stride;
  a.range_flag = dflag;
  a.Ah = (const uint16_t*)at(dAh, g->Ah); a.Al = (const uint16_t*)at(dAl, g->Al);
  a.Ch = (uint16_t*)at(dCh, g->Ch); a.Cl = (uint16_t*)at(dCl, g->Cl);

  int status;
  if (f16) {
    if (g->ldwt == K) wb::launch_split_weight_f16(nullptr, (const float*)dW, (int)K, (int)N, (uint16_t*)dWh, (uint16_t*)dWl);
    status = wb::launch_gemm_f16x3(nullptr, a, (const uint16_t*)dWh, (const uint16_t*)dWl, (int)g->ldwt);
  } else {
    status = wb::launch_gemm_f32(nullptr, a);
  }
  status = finish(P, status);
  if (status < -999) return status;
  download(P, g->C, dC); download(P, g->Ch, dCh); download(P, g->Cl, dCl); download(P, g->Wh, dWh); download(P, g->Wl, dWl);
  g->range_flag_out = 0;
  if (dflag) { int v = 0; P.ok(hipMemcpy(&v, dflag, 4, hipMemcpyDeviceToHost)); g->range_flag_out = v; }
  return P.err ? P.err : status;
}

struct WbkAttn {
  int64_t which;                    // 0: launch_attention_f32, 1: launch_attention
  WbkBuf X;                         // f32 array holding Q, K and V (fused-QKV or cross views): off unused
  int64_t q_off, k_off, v_off;      // ELEMENT offsets of the three pointers in X
  WbkBuf O, Oh, Ol, segs;           // O / Oh / Ol copied in and back; segs: AttnSeg[n_segs]
  int64_t ldq, ldkv, ldo, n_segs, max_q_len, n_head, causal, split;
  int64_t wrote_pieces;             // out: launch_attention's return value
  double scale;
};

int wbk_attention(WbkAttn* t) {
  const int64_t H = t->n_head, hd = 64;
  if (t->n_segs < 1 || H < 1 || t->max_q_len < 1 || !t->X.host || t->X.off != 0 || !t->segs.host) return WBK_EARG;
  if (t->segs.off != 0 || t->segs.bytes < t->n_segs * (int64_t)sizeof(wb::AttnSeg)) return WBK_EARG;
  // the alignment contracts of kernels.h (rows are read and written as float4 / 8-byte piece groups)
  if (t->ldq % 4 || t->ldkv % 4 || t->ldo % 4 || t->q_off % 4 || t->k_off % 4 || t->v_off % 4) return WBK_EARG;
  if (t->ldq < H * hd || t->ldkv < H * hd || t->ldo < H * hd) return WBK_EARG;
  const bool pieces = t->Oh.host && t->Ol.host;
  if ((t->Oh.host != nullptr) != (t->Ol.host != nullptr)) return WBK_EARG;
  if (pieces && (t->Oh.bytes != t->Ol.bytes || t->Oh.off != t->Ol.off || (t->Oh.off & 7))) return WBK_EARG;
  if (!t->O.host || (t->O.off & 15)) return WBK_EARG;
  const wb::AttnSeg* s = (const wb::AttnSeg*)t->segs.host;
  const int64_t xe = t->X.bytes / 4;
  for (int64_t i = 0; i < t->n_segs; i++) {
    if (s[i].q_len < 0 || s[i].kv_len < 1 || s[i].q_len > t->max_q_len || s[i].q_row0 < 0 || s[i].kv_row0 < 0) return WBK_EARG;
    if (s[i].q_len == 0) continue;
    const int64_t qhi = t->q_off + (int64_t)(s[i].q_row0 + s[i].q_len - 1) * t->ldq + H * hd;
    const int64_t khi = (int64_t)(s[i].kv_row0 + s[i].kv_len - 1) * t->ldkv + H * hd;
    if (qhi > xe || t->k_off + khi > xe || t->v_off + khi > xe || t->q_off < 0 || t->k_off < 0 || t->v_off < 0) return WBK_EARG;
    const int64_t olo = (int64_t)s[i].q_row0 * t->ldo, ohi = (int64_t)(s[i].q_row0 + s[i].q_len - 1) * t->ldo + H * hd;
    if (!inside(t->O, olo, ohi, 4)) return WBK_EARG;
    if (pieces && !inside(t->Oh, olo, ohi, 2)) return WBK_EARG;
  }
  Pool P;
  char *dX = upload(P, t->X), *dO = upload(P, t->O), *dOh = upload(P, t->Oh), *dOl = upload(P, t->Ol), *dS = upload(P, t->segs);
  if (P.err) return P.err;
  const float* X = (const float*)dX;
  float* O = (float*)(dO + t->O.off);
  uint16_t* Oh = pieces ? (uint16_t*)(dOh + t->Oh.off) : nullptr;
  uint16_t* Ol = pieces ? (uint16_t*)(dOl + t->Ol.off) : nullptr;
  t->wrote_pieces = 0;
  if (t->which == 0) {
    wb::launch_attention_f32(nullptr, X + t->q_off, (int)t->ldq, X + t->k_off, X + t->v_off, (int)t->ldkv, O, (int)t->ldo,
                             (const wb::AttnSeg*)dS, (int)t->n_segs, (int)t->max_q_len, (int)H, (float)t->scale, (int)t->causal);
  } else {
    t->wrote_pieces = wb::launch_attention(nullptr, X + t->q_off, (int)t->ldq, X + t->k_off, X + t->v_off, (int)t->ldkv, O,
                                           (int)t->ldo, (const wb::AttnSeg*)dS, (int)t->n_segs, (int)t->max_q_len, (int)H,
                                           (float)t->scale, (int)t->causal, t->split != 0, Oh, Ol) ? 1 : 0;
  }
  const int status = finish(P, 0);
  if (status) return status;
  download(P, t->O, dO); download(P, t->Oh, dOh); download(P, t->Ol, dOl);
  return P.err;
}

struct WbkNorm {
  int64_t which;                    // 0: launch_layernorm, 1: launch_layernorm_pieces, 2: launch_embed
  WbkBuf x, g, b;                   // LayerNorm: x [M][d], g [d], b [d].  embed: x = E [n_vocab][d], g = pos [L][d], b = tok (int32 [M])
  WbkBuf y, yh, yl;                 // outputs (copied in and back): y f32, or the pieces
  int64_t M, d, eps_inside_sqrt, L, n_vocab;
  double eps;
};

int wbk_norm(WbkNorm* t) {
  const int64_t M = t->M, d = t->d;
  if (M < 1 || d < 1 || M > (1 << 20) || d > (1 << 20)) return WBK_EARG;
  if (d % 4 != 0) return WBK_EARG;                              // kernels.h: rows are read as float4
  Pool P;
  if (t->which == 2) {
    const int32_t* tok = (const int32_t*)t->b.host;
    if (!tok || t->b.off != 0 || t->b.bytes < M * 4 || t->L < 1 || t->n_vocab < 1) return WBK_EARG;
    for (int64_t r = 0; r < M; r++) if (tok[r] < 0 || tok[r] >= t->n_vocab) return WBK_EARG;
    if (!inside(t->x, 0, t->n_vocab * d, 4) || !inside(t->g, 0, std::min(M, t->L) * d, 4) || !inside(t->y, 0, M * d, 4)) return WBK_EARG;
    if (!aligned16(t->x, 0, 4) || !aligned16(t->g, 0, 4) || !aligned16(t->y, 0, 4)) return WBK_EARG;
    char *dE = upload(P, t->x), *dpos = upload(P, t->g), *dtok = upload(P, t->b), *dy = upload(P, t->y);
    if (P.err) return P.err;
    wb::launch_embed(nullptr, (const int32_t*)dtok, (int)M, (int)t->L, (int)d, (const float*)(dE + t->x.off),
                     (const float*)(dpos + t->g.off), (float*)(dy + t->y.off));
    const int status = finish(P, 0);
    if (status) return status;
    download(P, t->y, dy);
    return P.err;
  }
  if (!inside(t->x, 0, M * d, 4) || !inside(t->g, 0, d, 4) || !inside(t->b, 0, d, 4)) return WBK_EARG;
  if (!aligned16(t->x, 0, 4) || !aligned16(t->g, 0, 4) || !aligned16(t->b, 0, 4)) return WBK_EARG;
  if (t->which == 0) {
    if (!inside(t->y, 0, M * d, 4) || !aligned16(t->y, 0, 4)) return WBK_EARG;
  } else {
    if (!t->yl.host || t->yl.bytes != t->yh.bytes || t->yl.off != t->yh.off || !inside(t->yh, 0, M * d, 2) || (t->yh.off & 7))
      return WBK_EARG;
  }
  char *dx = upload(P, t->x), *dg = upload(P, t->g), *db = upload(P, t->b);
  char *dy = upload(P, t->y), *dyh = upload(P, t->yh), *dyl = upload(P, t->yl);
  if (P.err) return P.err;
  if (t->which == 0)
    wb::launch_layernorm(nullptr, (const float*)(dx + t->x.off), (float*)(dy + t->y.off), (int)M, (int)d,
                         (const float*)(dg + t->g.off), (const float*)(db + t->b.off), (float)t->eps, (int)t->eps_inside_sqrt);
  else
    wb::launch_layernorm_pieces(nullptr, (const float*)(dx + t->x.off), (uint16_t*)(dyh + t->yh.off), (uint16_t*)(dyl + t->yl.off),
                                (int)M, (int)d, (const float*)(dg + t->g.off), (const float*)(db + t->b.off), (float)t->eps,
                                (int)t->eps_inside_sqrt);
  const int status = finish(P, 0);
  if (status) return status;
  download(P, t->y, dy); download(P, t->yh, dyh); download(P, t->yl, dyl);
  return P.err;
}

struct WbkSkinny {
  WbkBuf A, B;                      // A [M][lda] f32, B [K][N] f32 dense (ldb == N)
  WbkBuf th, tl;                    // pieces variant (both non-null): made on the device from B by launch_split_weight_f16_tiles
                                    // ([N / 16][K / 32][4][16][8] fp16, exactly K * N halves each), copied back
  WbkBuf P;                         // split-K planes, copied in and back
  int64_t lda, M, N, K, ksplit, plane, use_range_flag, range_flag_out;
};

int wbk_skinny_ksplit(int K, int N, int max_ks, int max_rows) { return wb::skinny_ksplit(K, N, max_ks, max_rows); }
int wbk_skinny_supported(int M, int K, int N) { return wb::skinny_supported(M, K, N) ? 1 : 0; }

int wbk_skinny(WbkSkinny* t) {
  const int64_t M = t->M, N = t->N, K = t->K;
  if (M < 1 || M > 64 || N < 1 || K < 1 || N > (1 << 20) || K > (1 << 20) || t->ksplit < 1) return WBK_EARG;
  const bool pieces = t->th.host != nullptr;
  if (t->lda % 4 || t->lda < K || !inside(t->A, 0, (M - 1) * t->lda + K, 4) || !aligned16(t->A, 0, 4)) return WBK_EARG;
  if (t->B.off != 0 || t->B.bytes != K * N * 4 || !t->B.host) return WBK_EARG;
  if (t->plane < M * N || !inside(t->P, 0, (t->ksplit - 1) * t->plane + M * N, 4) || !aligned16(t->P, 0, 4) || t->plane % 4) return WBK_EARG;
  if (pieces && (K % 32 || N % 16 || !t->tl.host || t->th.off || t->tl.off || t->th.bytes != K * N * 2 || t->tl.bytes != K * N * 2))
    return WBK_EARG;
  Pool Pl;
  char *dA = upload(Pl, t->A), *dB = upload(Pl, t->B), *dth = upload(Pl, t->th), *dtl = upload(Pl, t->tl), *dP = upload(Pl, t->P);
  int* dflag = nullptr;
  if (t->use_range_flag) {
    void* p = nullptr;
    if (Pl.ok(hipMalloc(&p, 4))) { Pl.dev.push_back(p); Pl.ok(hipMemset(p, 0, 4)); dflag = (int*)p; }
  }
  if (Pl.err) return Pl.err;
  wb::SkinnyArgs a;
  a.A = (const float*)(dA + t->A.off); a.lda = (int)t->lda;
  a.B = (const float*)dB; a.ldb = (int)N;
  a.M = (int)M; a.N = (int)N; a.K = (int)K; a.ksplit = (int)t->ksplit;
  a.P = (float*)(dP + t->P.off); a.plane = (int)t->plane;
  a.range_flag = dflag;
  if (pieces) {
    wb::launch_split_weight_f16_tiles(nullptr, (const float*)dB, (int)K, (int)N, (uint16_t*)dth, (uint16_t*)dtl);
    a.Bh = (const uint16_t*)dth; a.Bl = (const uint16_t*)dtl;
  }
  int status = wb::launch_dec_skinny_gemm(nullptr, a);
  status = finish(Pl, status);
  if (status < -999) return status;
  download(Pl, t->P, dP); download(Pl, t->th, dth); download(Pl, t->tl, dtl);
  t->range_flag_out = 0;
  if (dflag) { int v = 0; Pl.ok(hipMemcpy(&v, dflag, 4, hipMemcpyDeviceToHost)); t->range_flag_out = v; }
  return Pl.err ? Pl.err : status;
}

// token alignment (align.hip).  stages bit 0: launch_align_row_stats, bit 1: launch_align_accumulate (reads `stats`: run both,
// or hand in the stats of an earlier call).  Q [n_q_rows][ldq], K [n_kv_rows][ldkv]; segs: wb::AttnSeg[n_rows]; heads: int32.
struct WbkAlign {
  WbkBuf Q, K, segs, heads, stats, M;
  int64_t ldq, ldkv, n_q_rows, n_kv_rows, n_rows, max_len, n_heads, n_model_heads, ld_stats, ld_row, ldm, filter_width, first,
      n_total, stages;
};

int wbk_align(WbkAlign* t) {
  const int64_t n = t->n_rows, nh = t->n_heads;
  if (n < 1 || n > 4096 || nh < 1 || nh > 4096 || t->max_len < 1 || t->max_len > wb::ALIGN_MAX_LEN) return WBK_EARG;
  if (t->ldq % 4 || t->ldkv % 4 || t->ldq < 64 * t->n_model_heads || t->ldkv < 64 * t->n_model_heads) return WBK_EARG;
  if (!inside(t->Q, 0, t->n_q_rows * t->ldq, 4) || !inside(t->K, 0, t->n_kv_rows * t->ldkv, 4)) return WBK_EARG;
  if (!aligned16(t->Q, 0, 4) || !aligned16(t->K, 0, 4)) return WBK_EARG;
  const wb::AttnSeg* sg = (const wb::AttnSeg*)t->segs.host;
  const int32_t* hd = (const int32_t*)t->heads.host;
  if (!sg || t->segs.off || t->segs.bytes < n * (int64_t)sizeof(wb::AttnSeg) || !hd || t->heads.off || t->heads.bytes < nh * 4)
    return WBK_EARG;
  for (int64_t h = 0; h < nh; h++) if (hd[h] < 0 || hd[h] >= t->n_model_heads) return WBK_EARG;
  int64_t max_C = 0;
  for (int64_t i = 0; i < n; i++) {
    if (sg[i].q_len < 1 || sg[i].q_len > t->max_len || sg[i].kv_len < 1 || sg[i].q_row0 < 0 || sg[i].kv_row0 < 0 ||
        sg[i].q_row0 + (int64_t)sg[i].q_len > t->n_q_rows || sg[i].kv_row0 + (int64_t)sg[i].kv_len > t->n_kv_rows)
      return WBK_EARG;
    if (sg[i].q_len > t->ld_stats || sg[i].q_len > t->ld_row || sg[i].kv_len > t->ldm) return WBK_EARG;
    max_C = std::max<int64_t>(max_C, sg[i].kv_len);
  }
  if (!inside(t->stats, 0, nh * n * t->ld_stats * 2, 4) || ((t->stats.off) & 7)) return WBK_EARG;
  if ((t->stages & 2) && !inside(t->M, 0, n * t->ld_row * t->ldm, 4)) return WBK_EARG;
  if ((t->stages & 2) && (t->filter_width < 1 || t->filter_width > 15 || !(t->filter_width & 1))) return WBK_EARG;
  Pool P;
  char *dQ = upload(P, t->Q), *dK = upload(P, t->K), *dS = upload(P, t->segs), *dH = upload(P, t->heads),
       *dst = upload(P, t->stats), *dM = upload(P, t->M);
  if (P.err) return P.err;
  int status = 0;
  if (t->stages & 1)
    wb::launch_align_row_stats(nullptr, (const float*)(dQ + t->Q.off), (int)t->ldq, (const float*)(dK + t->K.off), (int)t->ldkv,
                               (const wb::AttnSeg*)dS, (int)n, (int)t->max_len, (const int32_t*)dH, (int)nh,
                               (float2*)(dst + t->stats.off), (int)t->ld_stats);
  if (t->stages & 2)
    status = wb::launch_align_accumulate(nullptr, (const float*)(dQ + t->Q.off), (int)t->ldq, (const float*)(dK + t->K.off),
                                         (int)t->ldkv, (const wb::AttnSeg*)dS, (int)n, (int)t->max_len, (int)max_C,
                                         (const int32_t*)dH, (int)nh, (const float2*)(dst + t->stats.off), (int)t->ld_stats,
                                         (float*)(dM + t->M.off), (int)t->ld_row, (int)t->ldm, (int)t->filter_width,
                                         (int)t->first, (int)t->n_total);
  status = finish(P, status);
  if (status < -999) return status;
  download(P, t->stats, dst); download(P, t->M, dM);
  return P.err ? P.err : status;
}

// launch_align_dtw over one matrix X [N][ldx] (negate: X = -M); out [N]
struct WbkDtw { WbkBuf X, out; int64_t N, C, ldx, negate; };

int wbk_align_dtw(WbkDtw* t) {
  const int64_t N = t->N, C = t->C;
  if (N < 1 || C < 1 || C > (1 << 20) || t->ldx < C || !inside(t->X, 0, (N - 1) * t->ldx + C, 4) || !inside(t->out, 0, N, 4))
    return WBK_EARG;
  Pool P;
  char *dX = upload(P, t->X), *dout = upload(P, t->out);
  const int64_t ldt = (C + 3) / 4;
  const wb::DtwSeg seg{0, (int32_t)N, (int32_t)C, 0};
  void *dseg = nullptr, *dtr = nullptr;
  if (P.ok(hipMalloc(&dseg, sizeof(seg)))) { P.dev.push_back(dseg); P.ok(hipMemcpy(dseg, &seg, sizeof(seg), hipMemcpyHostToDevice)); }
  if (P.ok(hipMalloc(&dtr, (size_t)(N * ldt * 4)))) P.dev.push_back(dtr);
  if (P.err) return P.err;
  int status = wb::launch_align_dtw(nullptr, (const float*)(dX + t->X.off), (int)t->ldx, (int)t->negate, (const wb::DtwSeg*)dseg,
                                    1, (int)N, (uint32_t*)dtr, N * ldt, (int)ldt, (int32_t*)(dout + t->out.off));
  status = finish(P, status);
  if (status < -999) return status;
  download(P, t->out, dout);
  return P.err ? P.err : status;
}

// launch_dec_cross_fused (decode_fused.hip): one fused cross-attention sublayer step over n_rows live rows.  The step state is
// assembled here (st[ST_N] = n_rows, row r belongs to window row_win[r], no row dead).  x_in / x_out [S][d], pend [KSp][S][d],
// ckv: cached K | V rows (V of a key sits d floats behind its K), win_row0 / win_C [W], P [n_head][S][d] (copied in and back).
struct WbkCross {
  WbkBuf x_in, pend, pbias, x_out, ln_g, ln_b, Wq, bq, ckv, win_row0, win_C, row_win, Wo, P;
  int64_t S, W, d, n_head, KSp, ldkv, koff, n_pass, n_rows, ln_inside;
  double ln_eps, scale;
};

int wbk_cross_fused_ring() { return wb::CROSS_FUSED_MAX_C; }   // keys one pass of this build's ring holds

int wbk_cross_fused(WbkCross* t) {
  const int64_t S = t->S, W = t->W, d = t->d, H = t->n_head, n = t->n_rows;
  if (!wb::dec_fused_supported((int)d) || H * 64 != d || S < 1 || S > 64 || n < 1 || n > S || W < 1 || W > 64) return WBK_EARG;
  if (t->n_pass < 1 || t->n_pass > wb::CROSS_FUSED_MAX_PASSES || t->KSp < 0 || t->KSp > 64) return WBK_EARG;
  if (t->ldkv % 4 || t->koff % 4 || t->koff < 0 || t->ldkv < 2 * d || !aligned16(t->ckv, t->koff, 4)) return WBK_EARG;
  const int32_t* r0 = (const int32_t*)t->win_row0.host; const int32_t* wc = (const int32_t*)t->win_C.host;
  const int32_t* rw = (const int32_t*)t->row_win.host;
  if (!r0 || !wc || !rw || t->win_row0.off || t->win_C.off || t->row_win.off || t->win_row0.bytes < W * 4 || t->win_C.bytes < W * 4 ||
      t->row_win.bytes < n * 4)
    return WBK_EARG;
  for (int64_t w = 0; w < W; w++) {
    if (wc[w] < 1 || wc[w] > t->n_pass * wb::CROSS_FUSED_MAX_C || r0[w] < 0) return WBK_EARG;
    if (!inside(t->ckv, t->koff + (int64_t)r0[w] * t->ldkv, t->koff + ((int64_t)r0[w] + wc[w] - 1) * t->ldkv + 2 * d, 4)) return WBK_EARG;
    if (((int64_t)r0[w] + wc[w]) * t->ldkv + t->koff + 2 * d >= (1ll << 31)) return WBK_EARG;   // (32-bit row offsets)
  }
  for (int64_t r = 0; r < n; r++) if (rw[r] < 0 || rw[r] >= W) return WBK_EARG;
  if (!inside(t->x_in, 0, S * d, 4) || !inside(t->x_out, 0, S * d, 4) || !inside(t->P, 0, H * S * d, 4) || !aligned16(t->P, 0, 4))
    return WBK_EARG;
  if (t->KSp > 0 && (!inside(t->pend, 0, t->KSp * S * d, 4) || !inside(t->pbias, 0, d, 4))) return WBK_EARG;
  if (!inside(t->ln_g, 0, d, 4) || !inside(t->ln_b, 0, d, 4) || !inside(t->bq, 0, d, 4)) return WBK_EARG;
  if (!inside(t->Wq, 0, d * d, 4) || !inside(t->Wo, 0, d * d, 4) || !aligned16(t->Wq, 0, 4) || !aligned16(t->Wo, 0, 4)) return WBK_EARG;

  const wb::StepLayout lay = wb::make_step_layout((int)S, (int)W);
  std::vector<int32_t> st((size_t)lay.total, 0);
  st[wb::ST_N] = (int32_t)n;
  for (int64_t r = 0; r < n; r++) st[(size_t)(lay.win + r)] = rw[r];
  const WbkBuf stb{st.data(), (int64_t)st.size() * 4, 0};

  Pool P;
  char *dst = upload(P, stb), *dx = upload(P, t->x_in), *dpe = upload(P, t->pend), *dpb = upload(P, t->pbias), *dxo = upload(P, t->x_out);
  char *dg = upload(P, t->ln_g), *db = upload(P, t->ln_b), *dWq = upload(P, t->Wq), *dbq = upload(P, t->bq), *dkv = upload(P, t->ckv);
  char *dr0 = upload(P, t->win_row0), *dwc = upload(P, t->win_C), *dWo = upload(P, t->Wo), *dP = upload(P, t->P);
  if (P.err) return P.err;
  auto at = [](char* p, const WbkBuf& b) -> char* { return p ? p + b.off : nullptr; };
  wb::CrossFusedArgs a;
  a.st = (const int*)dst; a.lay = lay; a.S = (int)S; a.d = (int)d; a.n_head = (int)H;
  a.x_in = (const float*)at(dx, t->x_in); a.pend = t->KSp > 0 ? (const float*)at(dpe, t->pend) : nullptr; a.KSp = (int)t->KSp;
  a.pbias = t->KSp > 0 ? (const float*)at(dpb, t->pbias) : nullptr; a.x_out = (float*)at(dxo, t->x_out);
  a.ln_g = (const float*)at(dg, t->ln_g); a.ln_b = (const float*)at(db, t->ln_b); a.ln_eps = (float)t->ln_eps; a.ln_inside = (int)t->ln_inside;
  a.Wq = (const float*)at(dWq, t->Wq); a.bq = (const float*)at(dbq, t->bq); a.scale = (float)t->scale;
  a.ckv = (const float*)at(dkv, t->ckv); a.ldkv = (int)t->ldkv; a.koff = (int)t->koff;
  a.win_row0 = (const int*)dr0; a.win_C = (const int*)dwc; a.n_pass = (int)t->n_pass;
  a.Wo = (const float*)at(dWo, t->Wo); a.P = (float*)at(dP, t->P);
  wb::launch_dec_cross_fused(nullptr, a, (int)n);
  const int status = finish(P, 0);
  if (status) return status;
  download(P, t->x_out, dxo); download(P, t->P, dP);
  return P.err;
}

// launch_dec_attn_fused_rounds (decode_fused.hip): one fused self-attention sublayer step at d = 384 over n_rows live rows, with
// n_reg (2 or 4) QKV weight rounds held in registers.  The step state is assembled here (st[ST_N] = n_rows, row r has length
// lens[r] including the new token, no row dead, step parity 0).  x_in / x_out [S][d], pend [KSp][S][d], Wqkv [d][ldqkv],
// tabs [S][Lmax]: cache slot of position p of row r; Kc / Vc [n_slots][d] (copied in and back: the new token's rows are
// written), P [n_head][S][d] (copied in and back).
struct WbkAttnRounds {
  WbkBuf x_in, pend, pbias, x_out, ln_g, ln_b, Wqkv, bqkv, Kc, Vc, tabs, lens, Wo, P;
  int64_t S, d, n_head, KSp, ldqkv, Lmax, n_slots, n_rows, ln_inside, n_reg;
  double ln_eps, scale;
};

int wbk_attn_fused(WbkAttnRounds* t) {
  const int64_t S = t->S, d = t->d, H = t->n_head, n = t->n_rows, Lmax = t->Lmax, NS = t->n_slots;
  if (d != 384 || H * 64 != d || S < 1 || S > 64 || n < 1 || n > S || t->KSp < 0 || t->KSp > 64) return WBK_EARG;
  if (t->n_reg != 2 && t->n_reg != 4) return WBK_EARG;
  if (Lmax < 1 || Lmax > 448 || NS < 1 || NS * d >= (1ll << 31)) return WBK_EARG;          // (448: the body's position arrays)
  if (t->ldqkv < 3 * d || t->ldqkv % 4 || !aligned16(t->Wqkv, 0, 4) || !inside(t->Wqkv, 0, (d - 1) * t->ldqkv + 3 * d, 4)) return WBK_EARG;
  const int32_t* tb = (const int32_t*)t->tabs.host; const int32_t* ln = (const int32_t*)t->lens.host;
  if (!tb || !ln || t->tabs.off || t->lens.off || t->tabs.bytes < S * Lmax * 4 || t->lens.bytes < n * 4) return WBK_EARG;
  std::vector<char> is_new((size_t)NS, 0);
  for (int64_t r = 0; r < n; r++) {
    if (ln[r] < 1 || ln[r] > Lmax) return WBK_EARG;
    for (int64_t p = 0; p < ln[r]; p++) if (tb[r * Lmax + p] < 0 || tb[r * Lmax + p] >= NS) return WBK_EARG;
    char& nw = is_new[(size_t)tb[r * Lmax + ln[r] - 1]];
    if (nw) return WBK_EARG;                                                               // (two rows writing one cache row)
    nw = 1;
  }
  if (!inside(t->Kc, 0, NS * d, 4) || !inside(t->Vc, 0, NS * d, 4) || !aligned16(t->Kc, 0, 4) || !aligned16(t->Vc, 0, 4)) return WBK_EARG;
  if (!inside(t->x_in, 0, S * d, 4) || !inside(t->x_out, 0, S * d, 4) || !inside(t->P, 0, H * S * d, 4) || !aligned16(t->P, 0, 4))
    return WBK_EARG;
  if (t->KSp > 0 && (!inside(t->pend, 0, t->KSp * S * d, 4) || !inside(t->pbias, 0, d, 4))) return WBK_EARG;
  if (!inside(t->ln_g, 0, d, 4) || !inside(t->ln_b, 0, d, 4) || !inside(t->bqkv, 0, 3 * d, 4)) return WBK_EARG;
  if (!inside(t->Wo, 0, d * d, 4) || !aligned16(t->Wo, 0, 4)) return WBK_EARG;

  const wb::StepLayout lay = wb::make_step_layout((int)S, 1);
  std::vector<int32_t> st((size_t)lay.total, 0);
  st[wb::ST_N] = (int32_t)n;
  for (int64_t r = 0; r < n; r++) st[(size_t)(lay.len + r)] = ln[r];
  const WbkBuf stb{st.data(), (int64_t)st.size() * 4, 0};

  Pool P;
  char *dst = upload(P, stb), *dx = upload(P, t->x_in), *dpe = upload(P, t->pend), *dpb = upload(P, t->pbias), *dxo = upload(P, t->x_out);
  char *dg = upload(P, t->ln_g), *db = upload(P, t->ln_b), *dW = upload(P, t->Wqkv), *dbq = upload(P, t->bqkv);
  char *dK = upload(P, t->Kc), *dV = upload(P, t->Vc), *dtb = upload(P, t->tabs), *dWo = upload(P, t->Wo), *dP = upload(P, t->P);
  if (P.err) return P.err;
  auto at = [](char* p, const WbkBuf& b) -> char* { return p ? p + b.off : nullptr; };
  wb::AttnFusedArgs a;
  a.st = (const int*)dst; a.lay = lay; a.S = (int)S; a.d = (int)d; a.n_head = (int)H;
  a.x_in = (const float*)at(dx, t->x_in); a.pend = t->KSp > 0 ? (const float*)at(dpe, t->pend) : nullptr; a.KSp = (int)t->KSp;
  a.pbias = t->KSp > 0 ? (const float*)at(dpb, t->pbias) : nullptr; a.x_out = (float*)at(dxo, t->x_out);
  a.ln_g = (const float*)at(dg, t->ln_g); a.ln_b = (const float*)at(db, t->ln_b); a.ln_eps = (float)t->ln_eps; a.ln_inside = (int)t->ln_inside;
  a.Wqkv = (const float*)at(dW, t->Wqkv); a.ldqkv = (int)t->ldqkv; a.bqkv = (const float*)at(dbq, t->bqkv); a.scale = (float)t->scale;
  a.Kc = (float*)at(dK, t->Kc); a.Vc = (float*)at(dV, t->Vc); a.tabs = (const int*)dtb; a.Lmax = (int)Lmax;
  a.Wo = (const float*)at(dWo, t->Wo); a.P = (float*)at(dP, t->P);
  int status = wb::launch_dec_attn_fused_rounds(nullptr, a, (int)n, (int)t->n_reg);
  status = finish(P, status);
  if (status) return status;
  download(P, t->x_out, dxo); download(P, t->P, dP); download(P, t->Kc, dK); download(P, t->Vc, dV);
  return P.err;
}

// launch_ps_pick_test (decode_persist.hip): the token pick of the persistent kernel's first-layer self-attention role over one
// row's tile records.  rec: n_tiles records of 16 bytes {tag, value (f32), tag, id (i32)}, 16-byte aligned in its array; every
// record must carry `tag` twice (a stale record would be waited for: refused here, nothing is launched).  out_id: the id.
struct WbkPick { WbkBuf rec; int64_t n_tiles, tag, out_id; };

int wbk_persist_pick(WbkPick* t) {
  const int64_t n = t->n_tiles;
  if (n < 1 || n > (1 << 20) || t->tag < 1 || t->tag > 0xffffffffll) return WBK_EARG;
  if (!inside(t->rec, 0, n * 4, 4) || !aligned16(t->rec, 0, 4)) return WBK_EARG;
  const uint32_t* hr = (const uint32_t*)((const char*)t->rec.host + t->rec.off);
  for (int64_t i = 0; i < n; i++) if (hr[4 * i] != (uint32_t)t->tag || hr[4 * i + 2] != (uint32_t)t->tag) return WBK_EARG;
  Pool P;
  char* drec = upload(P, t->rec);
  const int n_ctl = wb::ps_ctl_ints(1, 1);
  void *dctl = nullptr, *dout = nullptr;
  if (P.ok(hipMalloc(&dctl, (size_t)n_ctl * 4))) { P.dev.push_back(dctl); P.ok(hipMemset(dctl, 0, (size_t)n_ctl * 4)); }
  if (P.ok(hipMalloc(&dout, 4))) { P.dev.push_back(dout); P.ok(hipMemset(dout, 0xff, 4)); }
  if (P.err) return P.err;
  wb::launch_ps_pick_test(nullptr, drec + t->rec.off, (int)n, (unsigned)t->tag, (int*)dctl, (int*)dout);
  const int status = finish(P, 0);
  if (status) return status;
  int id = -1;
  P.ok(hipMemcpy(&id, dout, 4, hipMemcpyDeviceToHost));
  t->out_id = id;
  return P.err;
}

// launch_ps_mlp2_test (decode_persist.hip) next to launch_dec_mlp_fused (decode_fused.hip) on the same inputs: one layer's MLP
// over n_rows <= 4 rows (S = n_rows).  x_in [S][d], pend [KSp][S][d] (the cross-attention planes), pbias [d], W1 [d][ld1], b1 [4 d],
// W2 [4 d][d], b2 [d], dead [S] int32 (two-phase form only: != 0 masks the row).  Out: rows2 [S][d] + tags2 [S][d] (uint32) = the
// two-phase roles' finished rows and their granule tags (tag_out = tag_in + 1 where a row was written, 0 elsewhere); P
// [4 d / 64][S][d] and x_out [S][d] = what the one-launch kernel leaves (the consumer folds x_out + (b2 + sum_j P[j])).
struct WbkMlp2 {
  WbkBuf x_in, pend, pbias, ln_g, ln_b, W1, b1, W2, b2, dead, rows2, tags2, P, x_out;
  int64_t S, d, KSp, ld1, ln_inside, tag_in;
  double ln_eps;
};

int wbk_persist_mlp2(WbkMlp2* t) {
  const int64_t S = t->S, d = t->d, K = t->KSp, NB = 4 * d / 64;
  if ((d != 128 && d != 384) || S < 1 || S > 4 || K < 1 || K > 8 || t->ld1 < 4 * d || t->ld1 % 4) return WBK_EARG;
  if (t->tag_in < 1 || t->tag_in > 0xfffffff0ll) return WBK_EARG;
  if (!inside(t->x_in, 0, S * d, 4) || !inside(t->pend, 0, K * S * d, 4) || !inside(t->pbias, 0, d, 4)) return WBK_EARG;
  if (!inside(t->ln_g, 0, d, 4) || !inside(t->ln_b, 0, d, 4) || !inside(t->b1, 0, 4 * d, 4) || !inside(t->b2, 0, d, 4)) return WBK_EARG;
  if (!inside(t->W1, 0, (d - 1) * t->ld1 + 4 * d, 4) || !aligned16(t->W1, 0, 4) || !inside(t->W2, 0, 4 * d * d, 4) || !aligned16(t->W2, 0, 4)) return WBK_EARG;
  if (!inside(t->dead, 0, S, 4) || !inside(t->rows2, 0, S * d, 4) || !inside(t->tags2, 0, S * d, 4)) return WBK_EARG;
  if (!inside(t->P, 0, NB * S * d, 4) || !aligned16(t->P, 0, 4) || !inside(t->x_out, 0, S * d, 4)) return WBK_EARG;
  // the role's inputs as {tag, value} granules
  auto granules = [&](const WbkBuf& b, int64_t n) {
    std::vector<uint32_t> g((size_t)n * 2);
    const uint32_t* v = (const uint32_t*)((const char*)b.host + b.off);
    for (int64_t i = 0; i < n; i++) { g[2 * i] = (uint32_t)t->tag_in; g[2 * i + 1] = v[i]; }
    return g;
  };
  std::vector<uint32_t> gx = granules(t->x_in, S * d), gp = granules(t->pend, K * S * d);
  std::vector<uint32_t> gout((size_t)(S + 8) * d * 2, 0u), ghid((size_t)(S + 2) * 4 * d * 2, 0u);
  std::vector<int32_t> ctl((size_t)wb::ps_ctl_ints(1, 1), 0);
  const wb::StepLayout lay = wb::make_step_layout((int)S, 1);
  std::vector<int32_t> st((size_t)lay.total, 0);
  st[wb::ST_N] = (int32_t)S;
  auto vb = [](auto& v) { return WbkBuf{v.data(), (int64_t)(v.size() * sizeof(v[0])), 0}; };
  const WbkBuf gxb = vb(gx), gpb = vb(gp), goutb = vb(gout), ghidb = vb(ghid), ctlb = vb(ctl), stb = vb(st);

  Pool P;
  char *dx = upload(P, t->x_in), *dpe = upload(P, t->pend), *dpb = upload(P, t->pbias), *dg = upload(P, t->ln_g), *db = upload(P, t->ln_b);
  char *dW1 = upload(P, t->W1), *db1 = upload(P, t->b1), *dW2 = upload(P, t->W2), *db2 = upload(P, t->b2), *ddead = upload(P, t->dead);
  char *dP = upload(P, t->P), *dxo = upload(P, t->x_out);
  char *dgx = upload(P, gxb), *dgp = upload(P, gpb), *dgo = upload(P, goutb), *dgh = upload(P, ghidb), *dctl = upload(P, ctlb), *dst = upload(P, stb);
  if (P.err) return P.err;
  auto at = [](char* p, const WbkBuf& b) -> char* { return p ? p + b.off : nullptr; };
  wb::MlpFusedArgs a;
  a.st = (const int*)dst; a.S = (int)S; a.d = (int)d;
  a.x_in = (const float*)at(dx, t->x_in); a.pend = (const float*)at(dpe, t->pend); a.KSp = (int)K; a.pbias = (const float*)at(dpb, t->pbias);
  a.x_out = (float*)at(dxo, t->x_out);
  a.ln_g = (const float*)at(dg, t->ln_g); a.ln_b = (const float*)at(db, t->ln_b); a.ln_eps = (float)t->ln_eps; a.ln_inside = (int)t->ln_inside;
  a.W1 = (const float*)at(dW1, t->W1); a.ld1 = (int)t->ld1; a.b1 = (const float*)at(db1, t->b1); a.W2 = (const float*)at(dW2, t->W2);
  a.P = (float*)at(dP, t->P);
  a.g_x_in = dgx; a.g_pend = dgp; a.g_x_out = dgo; a.g_P = nullptr;
  wb::launch_dec_mlp_fused(nullptr, a, (int)S);
  int status = finish(P, 0);
  if (status) return status;
  wb::PsMlp2TestArgs ta;
  ta.a = a; ta.n_rows = (int)S; ta.dead = (const int*)at(ddead, t->dead); ta.g_hid = dgh; ta.b2 = (const float*)at(db2, t->b2);
  ta.tag_in = (unsigned)t->tag_in; ta.ctl = (int*)dctl;
  status = finish(P, wb::launch_ps_mlp2_test(nullptr, ta));
  if (status) return status;
  download(P, t->P, dP); download(P, t->x_out, dxo); download(P, goutb, dgo);
  uint32_t* r2 = (uint32_t*)((char*)t->rows2.host + t->rows2.off); uint32_t* t2 = (uint32_t*)((char*)t->tags2.host + t->tags2.off);
  for (int64_t i = 0; i < S * d; i++) { t2[i] = gout[2 * i]; r2[i] = gout[2 * i + 1]; }
  return P.err;
}

// launch_ps_logits_test (decode_persist.hip): ONE logits role of the persistent kernel over tiles 0 .. n_t - 1 and n_rows <= 4 rows
// (S = n_rows).  x [S][d]: the last layer's finished rows; ln_g / ln_b [d]; Et [d][vocab_ld] (vocab_ld % 4 == 0, >= 128 n_t);
// dead [S] int32.  mlp2 = 1: the role takes the rows as granules and normalises them itself.  mlp2 = 0: the final-LN role of every
// row runs first (no planes to fold, a zero bias: it leaves ln(x + 0)), then the logits role on its rows.  rec: [S][n_t] records of
// 16 bytes {tag, value, tag, id}, zero where nothing was stored.
struct WbkLogits {
  WbkBuf x, ln_g, ln_b, Et, dead, rec;
  int64_t S, d, V, vocab_ld, n_t, ln_inside, tag, mlp2;
  double ln_eps;
};

int wbk_persist_logits(WbkLogits* t) {
  const int64_t S = t->S, d = t->d, nt = t->n_t, ld = t->vocab_ld;
  if ((d != 128 && d != 384) || S < 1 || S > 4 || nt < 1 || nt > 2 || ld % 4 || ld < 128 * nt || t->V < 1 || t->V > ld) return WBK_EARG;
  if ((t->V + 127) / 128 != nt || t->tag < 1 || t->tag > 0xfffffff0ll || (t->mlp2 != 0 && t->mlp2 != 1)) return WBK_EARG;
  if (!inside(t->x, 0, S * d, 4) || !inside(t->ln_g, 0, d, 4) || !inside(t->ln_b, 0, d, 4) || !inside(t->dead, 0, S, 4)) return WBK_EARG;
  if (!inside(t->Et, 0, d * ld, 4) || !aligned16(t->Et, 0, 4) || !inside(t->rec, 0, S * nt * 4, 4) || !aligned16(t->rec, 0, 4)) return WBK_EARG;
  std::vector<uint32_t> gx((size_t)(S + 8) * d * 2, 0u), gxn((size_t)(S + 8) * d * 2, 0u);
  const uint32_t* xv = (const uint32_t*)((const char*)t->x.host + t->x.off);
  for (int64_t i = 0; i < S * d; i++) { gx[2 * i] = (uint32_t)t->tag; gx[2 * i + 1] = xv[i]; }
  std::vector<float> zero((size_t)d, 0.f);
  std::vector<uint32_t> rec((size_t)S * nt * 4, 0u);
  std::vector<int32_t> ctl((size_t)wb::ps_ctl_ints(1, 1), 0);
  auto vb = [](auto& v) { return WbkBuf{v.data(), (int64_t)(v.size() * sizeof(v[0])), 0}; };
  const WbkBuf gxb = vb(gx), gxnb = vb(gxn), zb = vb(zero), recb = vb(rec), ctlb = vb(ctl);
  Pool P;
  char *dg = upload(P, t->ln_g), *db = upload(P, t->ln_b), *dE = upload(P, t->Et), *ddead = upload(P, t->dead);
  char *dgx = upload(P, gxb), *dgxn = upload(P, gxnb), *dz = upload(P, zb), *drec = upload(P, recb), *dctl = upload(P, ctlb);
  if (P.err) return P.err;
  auto at = [](char* p, const WbkBuf& b) -> char* { return p ? p + b.off : nullptr; };
  wb::PersistArgs a;
  a.n_rows = (int)S; a.S = (int)S; a.d = (int)d; a.nb_mlp = 0; a.ctl = (int*)dctl; a.mask_until_len = -4;
  a.x_fin = dgx; a.P2 = dgx; a.b2_last = (const float*)dz; a.g_xn = dgxn;
  a.ln_g = (const float*)at(dg, t->ln_g); a.ln_b = (const float*)at(db, t->ln_b); a.ln_eps = (float)t->ln_eps; a.ln_inside = (int)t->ln_inside;
  a.Et = (const float*)at(dE, t->Et); a.vocab_ld = (int)ld; a.V = (int)t->V; a.mask = nullptr;
  a.tstats = drec; a.n_tiles = (int)nt; a.mlp2 = (int)t->mlp2; a.dead = (int*)at(ddead, t->dead);
  const int status = finish(P, wb::launch_ps_logits_test(nullptr, a, (unsigned)t->tag, (int)nt));
  if (status) return status;
  download(P, recb, drec);
  memcpy((char*)t->rec.host + t->rec.off, rec.data(), rec.size() * 4);
  return P.err;
}

const char* wbk_version() { return "whisper_hip kernel test harness 1"; }

}  // extern "C"
