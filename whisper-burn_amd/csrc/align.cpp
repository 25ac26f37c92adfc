// C ABI of the token alignment: cross-attention weights of a few heads -> token x position matrix -> DTW start positions
// (kernels: align.hip, the teacher-forced pass: engine.cpp run_align).
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>

#include "engine.h"
#include "session.h"

namespace wb {

// heads (n_heads pairs (layer, head); null / 0: every head of the upper half of the decoder) -> job, layers ascending
static int align_heads(const wb_model* m, const int32_t* heads, int32_t n_heads, AlignJob* J) {
  const int NL = m->dims.n_text_layer, H = m->dims.n_text_head;
  std::vector<std::pair<int32_t, int32_t>> hs;
  if (!heads || n_heads <= 0) {
    WB_REQUIRE(!heads && n_heads == 0, WB_ERR_ARG, "align: heads and n_heads must both be given, or neither");
    for (int l = NL / 2; l < NL; l++)
      for (int h = 0; h < H; h++) hs.emplace_back(l, h);
  } else {
    for (int i = 0; i < n_heads; i++) {
      const int32_t l = heads[2 * i], h = heads[2 * i + 1];
      WB_REQUIRE(l >= 0 && l < NL && h >= 0 && h < H, WB_ERR_ARG, "align: head (%d, %d) outside %d layers x %d heads", l, h,
                 NL, H);
      // (each pair once: a layer then owns at most n_text_head heads, which is what the statistics buffer holds)
      for (const auto& p : hs)
        WB_REQUIRE(p.first != l || p.second != h, WB_ERR_ARG, "align: head (%d, %d) is listed twice", l, h);
      hs.emplace_back(l, h);
    }
  }
  // the teacher-forced pass meets the layers in order; heads of one layer keep the caller's order
  std::stable_sort(hs.begin(), hs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  J->head_layer.clear(); J->head_id.clear();
  for (auto& p : hs) { J->head_layer.push_back(p.first); J->head_id.push_back(p.second); }
  return WB_OK;
}

// tokens [n][stride] + lens -> compact job rows; validates every argument that does not depend on the K source
// allow_empty: a row may leave no DTW row (n_prefix + drop_last >= len): it takes part in the pass and gets no position
static int align_rows(const wb_model* m, const int32_t* tokens, int n, int stride, const int32_t* lens, int32_t n_prefix,
                      int32_t drop_last, int32_t filter_width, AlignJob* J, bool allow_empty = false) {
  const int V = m->dims.n_vocab;
  WB_REQUIRE(filter_width >= 1 && filter_width <= 15 && (filter_width & 1), WB_ERR_ARG,
             "align: filter_width %d must be odd and in 1 .. 15", filter_width);
  WB_REQUIRE(n_prefix >= 0 && (drop_last == 0 || drop_last == 1), WB_ERR_ARG, "align: n_prefix %d / drop_last %d", n_prefix,
             drop_last);
  int L = 0;
  for (int i = 0; i < n; i++) {
    const int len = lens ? lens[i] : stride;
    WB_REQUIRE(len >= 1 && len <= stride, WB_ERR_ARG, "align: row %d has length %d (row stride %d)", i, len, stride);
    // mod.rs:134-139
    WB_REQUIRE(len <= m->dims.n_text_ctx && len <= ALIGN_MAX_LEN, WB_ERR_SHAPE,
               "Token sequence length %d must not exceed %d.", len, std::min((int)m->dims.n_text_ctx, ALIGN_MAX_LEN));
    WB_REQUIRE(allow_empty || n_prefix + drop_last < len, WB_ERR_ARG, "align: row %d: n_prefix %d + drop_last %d leave no token of %d", i,
               n_prefix, drop_last, len);
    L = std::max(L, len);
  }
  J->n = n; J->L = L;
  J->n_prefix = n_prefix; J->drop_last = drop_last; J->filter_width = filter_width;
  J->len.resize(n);
  J->tokens.assign((size_t)n * L, 0);
  for (int i = 0; i < n; i++) {
    J->len[i] = lens ? lens[i] : stride;
    for (int l = 0; l < J->len[i]; l++) {
      const int32_t t = tokens[(size_t)i * stride + l];
      WB_REQUIRE(t >= 0 && t < V, WB_ERR_ARG, "token id %d out of range [0,%d)", t, V);
      J->tokens[(size_t)i * L + l] = t;
    }
  }
  return WB_OK;
}

// enqueue the copies of the job's results into the caller's layout: start_pos [n][stride], matrix [n][stride][ldc]
static int align_fetch(hipStream_t st, const AlignBufs& B, const AlignJob& J, int stride, int ldc, int32_t* start_pos, float* matrix) {
  for (int i = 0; i < J.n; i++) {
    if (start_pos) {
      for (int l = 0; l < stride; l++) start_pos[(size_t)i * stride + l] = -1;
      WB_HIP(hipMemcpyAsync(start_pos + (size_t)i * stride, B.start.as<int32_t>() + (size_t)i * J.L, (size_t)J.len[i] * 4,
                            hipMemcpyDeviceToHost, st));
    }
    if (matrix) {
      memset(matrix + (size_t)i * stride * ldc, 0, (size_t)stride * ldc * 4);
      WB_HIP(hipMemcpy2DAsync(matrix + (size_t)i * stride * ldc, (size_t)ldc * 4, B.M.as<float>() + (size_t)i * J.L * J.maxC,
                              (size_t)J.maxC * 4, (size_t)J.C[i] * 4, (size_t)J.len[i], hipMemcpyDeviceToHost, st));
    }
  }
  return WB_OK;
}

int session_align(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, const int32_t* heads,
                  int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width, int32_t* start_pos,
                  float* matrix, const int32_t* drop_last_rows) {
  wb_model* m = s->m;
  WB_REQUIRE((int)s->C.size() == s->W && s->W > 0 && s->ckv.p, WB_ERR_STATE, "wb_session_align: the session holds no encoded windows");
  AlignJob J;
  WB_TRY(align_heads(m, heads, n_heads, &J));
  // (the transcription path hands in rows as decoded: one that is all prompt -- max_depth 0, a short mask -- gets no
  // position instead of failing the transcription)
  WB_TRY(align_rows(m, tokens, s->W, row_stride, lens, n_prefix, drop_last, filter_width, &J, drop_last_rows != nullptr));
  if (drop_last_rows) J.drop_rows.assign(drop_last_rows, drop_last_rows + s->W);
  wb::GpuTurn turn(s->device);
  WB_HIP(hipSetDevice(m->device));
  if (s->enc_guard_pending) {            // a deferred range check of the encode pass: settle it before its output is read
    WB_HIP(hipStreamSynchronize(s->st));
    bool reencoded = false;
    WB_TRY(session_enc_guard_resolve(s, &reencoded));
  }
  const int d = m->dims.n_text_state;
  J.C = s->C; J.kv_row0 = s->row0;
  J.ckv = s->ckv.as<float>(); J.ckv_layer_stride = (int64_t)s->enc_rows * 2 * d; J.ldkv = 2 * d;
  WB_TRY(run_align(m, s->st, s->ws, J));
  WB_TRY(align_fetch(s->st, s->ws.align, J, row_stride, s->maxC, start_pos, matrix));
  WB_HIP(hipStreamSynchronize(s->st));
  return WB_OK;
}

}  // namespace wb

using namespace wb;

extern "C" {

int wb_align_tokens(wb_model* m, const int32_t* tokens, int n, int L, const int32_t* lens, const float* enc, int C,
                    const int32_t* heads, int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width,
                    int32_t* start_pos, float* matrix) {
  WB_REQUIRE(m && tokens && enc && start_pos && n > 0 && L > 0 && C > 0, WB_ERR_ARG, "wb_align_tokens: bad argument");
  AlignJob J;
  WB_TRY(align_heads(m, heads, n_heads, &J));
  WB_TRY(align_rows(m, tokens, n, L, lens, n_prefix, drop_last, filter_width, &J));
  wb::GpuTurn turn(m->device);
  std::lock_guard<std::mutex> lk(g_stateless_mu);
  WB_HIP(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const int d = m->dims.n_text_state;
  WB_TRY(m->io_b.ensure((size_t)n * C * d * 4));
  WB_HIP(hipMemcpyAsync(m->io_b.p, enc, (size_t)n * C * d * 4, hipMemcpyHostToDevice, st));
  J.C.assign(n, C); J.kv_row0.resize(n);
  for (int i = 0; i < n; i++) J.kv_row0[i] = i * C;
  J.enc_dev = m->io_b.as<float>(); J.enc_rows = n * C;
  // (guarded: the cross-K projection runs on the split-precision kernel, as in wb_forward_decoder; the results are fetched
  // inside the pass so that the guard's synchronisation is the call's only one)
  WB_TRY(split_guarded(m, st, m->split_flag_host, m->split_flag_dev, nullptr, [&]() -> int {
    WB_TRY(run_align(m, st, m->ws, J));
    return align_fetch(st, m->ws.align, J, L, C, start_pos, matrix);
  }));
  WB_HIP(hipStreamSynchronize(st));      // (a model on the exact-f32 kernels runs the pass unguarded: nothing waited yet)
  return WB_OK;
}

int wb_session_align(wb_session* s, const int32_t* tokens, int32_t row_stride, const int32_t* lens, const int32_t* heads,
                     int32_t n_heads, int32_t n_prefix, int32_t drop_last, int32_t filter_width, int32_t* start_pos,
                     float* matrix) {
  WB_REQUIRE(s && tokens && start_pos && row_stride > 0, WB_ERR_ARG, "wb_session_align: bad argument");
  return session_align(s, tokens, row_stride, lens, heads, n_heads, n_prefix, drop_last, filter_width, start_pos, matrix,
                       nullptr);
}

int wb_dtw_start_positions(int device, const float* x, int32_t N, int32_t C, int32_t* start_pos) {
  WB_REQUIRE(x && start_pos && N >= 1 && C >= 1, WB_ERR_ARG, "wb_dtw_start_positions: bad argument");
  WB_REQUIRE(N <= 512 && C <= (1 << 20), WB_ERR_SHAPE, "wb_dtw_start_positions: %d x %d exceeds 512 rows / 2^20 columns", N, C);
  wb::GpuTurn turn(device);
  WB_HIP(hipSetDevice(device));
  const int ldt = (C + 3) / 4;
  DevMem dx, dseg, dtr, dout;
  WB_TRY(dx.alloc((size_t)N * C * 4));
  WB_TRY(dseg.alloc(sizeof(DtwSeg)));
  WB_TRY(dtr.alloc((size_t)N * ldt * 4));
  WB_TRY(dout.alloc((size_t)N * 4));
  const DtwSeg seg{0, N, C, 0};
  hipStream_t st = nullptr;
  WB_HIP(hipMemcpyAsync(dx.p, x, (size_t)N * C * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(dseg.p, &seg, sizeof(seg), hipMemcpyHostToDevice, st));
  prof_tag(KC_ALIGN_DTW, 0);
  WB_REQUIRE(launch_align_dtw(st, dx.as<float>(), C, 0, dseg.as<DtwSeg>(), 1, N, dtr.as<uint32_t>(), (int64_t)N * ldt, ldt,
                              dout.as<int32_t>()) == 0, WB_ERR_SHAPE, "wb_dtw_start_positions: unsupported shape");
  WB_HIP(hipGetLastError());
  WB_HIP(hipMemcpyAsync(start_pos, dout.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  return WB_OK;
}

int wb_stitch_windows_times(const int32_t* win_tokens, int32_t row_stride, const int32_t* win_lens, int n_windows,
                            int max_n_offsets, int min_n_overlaps, int32_t* out, int64_t cap, int64_t* n_out,
                            const float* win_times, float* out_times) {
  WB_REQUIRE(win_lens && out && n_out && win_times && out_times && (win_tokens || n_windows == 0), WB_ERR_ARG,
             "wb_stitch_windows_times: null argument");
  std::vector<int32_t> tokens;
  std::vector<float> times;
  for (int w = 0; w < n_windows; w++) {
    const int32_t* nt = win_tokens + (int64_t)w * row_stride;
    const float* tt = win_times + (int64_t)w * row_stride;
    const int64_t nn = win_lens[w];
    int64_t pi, ci;
    // transcribe.rs:56-63: prev[..prev_index] ++ curr[curr_index..]; a token keeps the time of the window it came from
    if (wb_find_chunk_overlap(tokens.data(), (int64_t)tokens.size(), nt, nn, max_n_offsets, min_n_overlaps, &pi, &ci)) {
      tokens.resize((size_t)pi); times.resize((size_t)pi);
      tokens.insert(tokens.end(), nt + ci, nt + nn); times.insert(times.end(), tt + ci, tt + nn);
    } else {
      tokens.insert(tokens.end(), nt, nt + nn); times.insert(times.end(), tt, tt + nn);
    }
  }
  WB_REQUIRE((int64_t)tokens.size() <= cap, WB_ERR_ARG, "wb_stitch_windows_times: output capacity %lld < %zu", (long long)cap,
             tokens.size());
  memcpy(out, tokens.data(), tokens.size() * sizeof(int32_t));
  memcpy(out_times, times.data(), times.size() * sizeof(float));
  *n_out = (int64_t)tokens.size();
  return WB_OK;
}

}  // extern "C"
