// Stateful session: one mel + encoder + cross-K/V pass per batch of windows, then KV-cached decode
// steps -- the result-equivalent fast path behind /root/reference/src/transcribe.rs:148-312.
#include "session.h"

#include <cstring>
#include <mutex>

#include "switches.h"

using namespace wb;

namespace wb {

// sessions are recycled per model so that a transcription loop does not pay hipMalloc per batch.
// g_pool has an entry for exactly the models that are alive: a session released after its model was freed is
// destroyed instead of being parked under a dangling key, and a pooled session never outlives its model.
static std::mutex g_pool_mu;
static std::unordered_map<uint64_t, std::vector<wb_session*>> g_pool;   // by wb_model::uid (never reused), not by address
static uint64_t g_next_model_uid = 1;
constexpr size_t POOL_MAX_SESSIONS = 8;
constexpr size_t POOL_MAX_BYTES = (size_t)4 << 30;   // per model: big batches (large-v2 x 64 windows ~ 20 GB) are not parked

void session_pool_register(wb_model* m) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  m->uid = g_next_model_uid++;
  g_pool[m->uid];
}

// wb_model_free: pooled sessions of that model die with it
void session_pool_purge(wb_model* m) {
  std::vector<wb_session*> dead;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.find(m->uid);
    if (it != g_pool.end()) { dead.swap(it->second); g_pool.erase(it); }
  }
  for (wb_session* s : dead) delete s;
}

static size_t session_device_bytes(const wb_session* s) {
  size_t n = 0;
  for (const DevMem* b : {&s->pcm, &s->mel, &s->wins, &s->gmax, &s->enc_out, &s->ckv, &s->win_meta, &s->kc, &s->vc,
                          &s->tabs, &s->state, &s->x, &s->h, &s->att, &s->Pqkv, &s->Po, &s->Pq, &s->P1, &s->P2, &s->Pa, &s->Pc, &s->carec, &s->ca,
                          &s->logits, &s->tstats, &s->row_stats, &s->mask, &s->lp_tmp, &s->gctl, &s->gtok, &s->hm,
                          &s->ws.x1, &s->ws.x, &s->ws.h, &s->ws.qkv, &s->ws.att, &s->ws.hm, &s->ws.desc1, &s->ws.desc2,
                          &s->ws.auxidx, &s->ws.segs, &s->ws.misc})
    n += b->bytes;
  return n;
}

int session_create(wb_model* m, int n_windows, int max_beams, int padding, wb_session** out) {
  WB_REQUIRE(m && out, WB_ERR_ARG, "session: null argument");
  WB_REQUIRE(n_windows >= 1, WB_ERR_ARG, "session: n_windows must be >= 1");
  WB_REQUIRE(max_beams >= 1 && max_beams <= MAX_BEAMS, WB_ERR_ARG, "session: max_beams must be in [1, %d]", MAX_BEAMS);
  WB_REQUIRE(padding >= 0 && padding < m->max_mel_frames(), WB_ERR_ARG, "session: bad padding %d", padding);
  WB_HIP(hipSetDevice(m->device));
  wb_session* s = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.find(m->uid);
    WB_REQUIRE(it != g_pool.end(), WB_ERR_ARG, "session: the model handle is not alive");
    if (!it->second.empty()) { s = it->second.back(); it->second.pop_back(); }
  }
  if (!s) {
    s = new wb_session();
    s->m = m;
    s->model_uid = m->uid;
    s->device = m->device;
    hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
    if (e != hipSuccess) { delete s; set_error("hipStreamCreate failed: %s", hipGetErrorString(e)); return WB_ERR_HIP; }
    e = hipHostMalloc((void**)&s->guard_host, 64, hipHostMallocMapped);
    if (e == hipSuccess) { memset(s->guard_host, 0, 64); e = hipHostGetDevicePointer((void**)&s->guard_dev, s->guard_host, 0); }
    if (e != hipSuccess) { delete s; set_error("session guard words: %s", hipGetErrorString(e)); return WB_ERR_HIP; }
  } else if (s->enc_guard_pending || s->guard_host[0] || s->guard_host[1]) {
    // a previous user left an unresolved guard behind (its call failed before the check): drain and clear
    (void)hipStreamSynchronize(s->st);
    s->guard_host[0] = s->guard_host[1] = 0;
  }
  s->enc_guard_pending = false;
  s->W = n_windows; s->max_beams = max_beams; s->S = n_windows * max_beams; s->padding = padding;
  s->T.assign(n_windows, 0); s->C.clear(); s->row0.clear();
  s->prev_len.clear(); s->prev_win.clear(); s->prev_n = 0; s->step = 0;
  s->has_mask = false; s->decode_ready = false; s->last_had_logits = 0; s->last_use_mask = 0;
  s->sample_rate = 16000.0;          // per-use state: a pooled session must not remember its previous caller
  s->smp_best_of = 0; s->smp_depth = 0; s->smp_len.clear(); s->smp_tokens.clear();
  s->has_suppress = false;
  s->prefill_mode = 0;
  *out = s;
  return WB_OK;
}

static int session_finish_encode(wb_session* s, const MelBatch& mb, bool defer_guard = false) {
  wb_model* m = s->m;
  const int d = m->dims.n_audio_state, NL = m->dims.n_text_layer;
  int rows = 0;
  for (int t : mb.T) rows += (t - 1) / 2 + 1;
  WB_TRY(s->enc_out.ensure((size_t)rows * d * 4));
  EncoderOut eo;
  const int rows_all = rows;
  const int ldkv_all = NL * 2 * d;
  WB_TRY(s->ckv.ensure((size_t)rows_all * ldkv_all * 4));
  // encoder + cross-K/V projection under ONE range guard of the split-precision kernel (engine.cpp: split_guarded), on
  // this session's own flag word; deferred: no synchronisation here, the decode's own resolves it
  bool deferred = false;
  WB_TRY(split_guarded(m, s->st, s->guard_host, s->guard_dev, defer_guard && !profile().on ? &deferred : nullptr, [&]() -> int {
  {
    ScopedTimer tm(s->st, 1);
    WB_TRY(run_encoder_unguarded(m, s->st, s->ws, mb, s->enc_out.as<float>(), &eo));
    tm.stop();
    if (tm.on) { WB_HIP(hipStreamSynchronize(s->st)); tm.collect(); }
  }
  {
    ScopedTimer tm(s->st, 2);
    GemmArgs g;
    // output layer-major: [layer][packed encoder row][K | V] -- one layer's cached K/V is one dense region (ckv_of)
    g.A = s->enc_out.as<float>(); g.lda = d; g.B = m->ckv_all.w; g.ldb = ldkv_all; g.C = s->ckv.as<float>(); g.ldc = 2 * d;
    g.c_block_cols = 2 * d; g.c_block_stride = (int64_t)rows_all * 2 * d;
    g.bias = m->ckv_all.b; g.M = rows_all; g.N = ldkv_all; g.K = d;
    g.col_scale = m->qk_scale; g.col_scale_period = 2 * d; g.col_scale_width = d;   // K * s (mod.rs:510-514)
    WB_TRY(gemm_dispatch(m, s->st, g, m->ckv_all.k, m->ckv_all.sh, m->ckv_all.sl));
    tm.stop();
    if (tm.on) { WB_HIP(hipStreamSynchronize(s->st)); tm.collect(); }
  }
  return WB_OK;
  }));
  s->enc_guard_pending = deferred;
  if (deferred) s->enc_mb = mb;
  s->C = eo.C; s->row0 = eo.row0; s->enc_rows = eo.rows;
  s->maxC = 0;
  for (int c : s->C) s->maxC = std::max(s->maxC, c);
  s->n_chunks = (s->maxC + cross_attn_chunk() - 1) / cross_attn_chunk();
  WB_REQUIRE(s->n_chunks <= CA_NCH_MAX, WB_ERR_SHAPE, "encoder context %d too long for the decode kernels", s->maxC);
  // (cross-attention K|V of every decoder layer, once per window -- mod.rs:484-485 does it per layer / beam / step -- ran
  // above, under the encoder's range guard)
  std::vector<int> meta(2 * s->W);
  for (int w = 0; w < s->W; w++) { meta[w] = s->row0[w]; meta[s->W + w] = s->C[w]; }
  WB_TRY(s->win_meta.ensure(meta.size() * 4));
  if (meta != s->meta_host || s->meta_dev_ptr != s->win_meta.p) {   // (same geometry as last time: already on the device)
    s->meta_host.clear(); s->meta_dev_ptr = nullptr;                 // void the cache key before the contents change
    WB_HIP(hipMemcpyAsync(s->win_meta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s->st));
    WB_HIP(hipStreamSynchronize(s->st));
    s->meta_host = meta; s->meta_dev_ptr = s->win_meta.p;
  }
  return WB_OK;
}

void session_rewind(wb_session* s) {
  s->prev_len.clear(); s->prev_win.clear(); s->prev_n = 0; s->step = 0;
  s->last_had_logits = 0; s->last_use_mask = 0; s->prof_step_off = 0;
}

// After s->st was synchronised behind a deferred encode pass: if the split-precision kernel raised this session's flag, the
// model has left that kernel and the pass is repeated here on the exact-f32 one (*reencoded = true: the encoder output and
// the cached cross K/V changed under whatever was decoded from them -- decode again).
int session_enc_guard_resolve(wb_session* s, bool* reencoded) {
  *reencoded = false;
  if (!s->enc_guard_pending) return WB_OK;
  s->enc_guard_pending = false;
  if (!split_guard_resolve(s->m, s->guard_host)) return WB_OK;
  *reencoded = true;
  return session_finish_encode(s, s->enc_mb, false);
}

int session_encode_pcm(wb_session* s, const float* pcm, int64_t n_pcm, const int64_t* starts, const int64_t* lens,
                       bool pcm_on_device, bool defer_guard) {
  wb_model* m = s->m;
  const int clip = m->max_mel_frames() - s->padding;   // transcribe.rs:171-177
  int64_t lo = n_pcm, hi = 0;
  for (int w = 0; w < s->W; w++) {
    WB_REQUIRE(starts[w] >= 0 && lens[w] >= 0 && starts[w] + lens[w] <= n_pcm, WB_ERR_ARG,
               "window %d [%lld, +%lld) outside the waveform (%lld samples)", w, (long long)starts[w],
               (long long)lens[w], (long long)n_pcm);
    WB_REQUIRE(lens[w] >= MEL_N_FFT, WB_ERR_SHAPE, "window %d has %lld samples < n_fft = 400 (audio.rs:292)", w,
               (long long)lens[w]);
    WB_REQUIRE(lens[w] < ((int64_t)1 << 30), WB_ERR_SHAPE, "window %d too long", w);
    lo = std::min(lo, starts[w]); hi = std::max(hi, starts[w] + lens[w]);
  }
  std::vector<MelWindow> wins(s->W);
  int maxF = 0, maxT = 0;
  for (int w = 0; w < s->W; w++) {
    const int nf = (int)(lens[w] / MEL_HOP);
    wins[w] = MelWindow{pcm_on_device ? starts[w] : starts[w] - lo, (int32_t)lens[w], nf, std::min(nf, clip), 0};
    s->T[w] = wins[w].n_emit + s->padding;
    maxF = std::max(maxF, nf); maxT = std::max(maxT, s->T[w]);
  }
  const int Ts = (maxT + 3) & ~3;
  MelFrontend fe;
  const int NMEL = m->dims.n_mels;
  WB_TRY(get_mel_frontend(m->device, s->sample_rate, __atomic_load_n(&m->frontend, __ATOMIC_RELAXED), NMEL, &fe));
  if (!pcm_on_device) WB_TRY(s->pcm.ensure((size_t)(hi - lo) * 4));
  WB_TRY(s->wins.ensure(wins.size() * sizeof(MelWindow)));
  WB_TRY(s->gmax.ensure((size_t)s->W * mel_bmax_stride(maxF) * 2 * 4));
  WB_TRY(s->mel.ensure((size_t)s->W * NMEL * Ts * 4));
  if (!pcm_on_device && sw::pcm_stage()) {
    const size_t nb = (size_t)(hi - lo) * 4;
    if (s->pcm_stage_bytes < nb) {
      if (s->pcm_stage) (void)hipHostFree(s->pcm_stage);
      s->pcm_stage = nullptr; s->pcm_stage_bytes = 0;
      WB_HIP(hipHostMalloc((void**)&s->pcm_stage, nb, hipHostMallocDefault));
      s->pcm_stage_bytes = nb;
    }
    memcpy(s->pcm_stage, pcm + lo, nb);
    WB_HIP(hipMemcpyAsync(s->pcm.p, s->pcm_stage, nb, hipMemcpyHostToDevice, s->st));
  } else
  if (!pcm_on_device) WB_HIP(hipMemcpyAsync(s->pcm.p, pcm + lo, (size_t)(hi - lo) * 4, hipMemcpyHostToDevice, s->st));
  const float* pcm_dev = pcm_on_device ? pcm : s->pcm.as<float>();
  // the window table on the device is re-used when this (pooled) session saw the same windows last time
  const bool same_wins = s->wins_host.size() == wins.size() && s->wins_dev_ptr == s->wins.p &&
                         memcmp(s->wins_host.data(), wins.data(), wins.size() * sizeof(MelWindow)) == 0;
  if (!same_wins) {
    s->wins_host.clear(); s->wins_dev_ptr = nullptr;                  // void the cache key before the contents change
    WB_HIP(hipMemcpyAsync(s->wins.p, wins.data(), wins.size() * sizeof(MelWindow), hipMemcpyHostToDevice, s->st));
    WB_HIP(hipStreamSynchronize(s->st));   // `wins` is a stack vector
    s->wins_host = wins; s->wins_dev_ptr = s->wins.p;
  } else if (!pcm_on_device) {
    WB_HIP(hipStreamSynchronize(s->st));   // the caller's PCM buffer may go away
  }
  const int trace_extra = sw::enc_trace_extra();
  if (!pcm_on_device && (trace_extra & 1)) enc_trace_stage(s->st, "pcm", s->pcm.p, (size_t)(hi - lo) * 4);
  {
    ScopedTimer tm(s->st, 0);
    launch_mel_frontend(s->st, fe, pcm_dev, s->wins.as<MelWindow>(), s->W, maxF, s->mel.as<float>(), (int64_t)NMEL * Ts, Ts,
                        s->gmax.as<float>(), s->padding, Ts, [&]() {
                          if (trace_extra & 2) enc_trace_stage(s->st, "mel0", s->mel.p, (size_t)s->W * NMEL * Ts * 4);
                          if (trace_extra & 4)
                            enc_trace_stage(s->st, "gmax", s->gmax.p, (size_t)s->W * mel_bmax_stride(maxF) * 2 * 4);
                        });
    tm.stop();
    if (tm.on) { WB_HIP(hipStreamSynchronize(s->st)); tm.collect(); profile().ms[5] += 1; }
  }
  WB_HIP(hipGetLastError());
  MelBatch mb;
  mb.mel = s->mel.as<float>(); mb.win_stride = (int64_t)NMEL * Ts; mb.row_stride = Ts; mb.T = s->T;
  return session_finish_encode(s, mb, defer_guard);
}

int session_reserve(wb_session* s, int max_len) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int d = D.n_text_state, NL = D.n_text_layer, V = D.n_vocab, S = s->S;
  WB_REQUIRE(d <= 1280, WB_ERR_SHAPE, "decode kernels keep whole rows in LDS: n_state %d > 1280", d);
  WB_REQUIRE(d % 64 == 0, WB_ERR_SHAPE, "decode kernels need n_state %% 64 == 0 (head size 64), got %d", d);
  max_len = std::max(8, std::min(max_len, std::min(D.n_text_ctx, 448)));
  s->Lmax = max_len;
  const size_t pool = (size_t)max_len * S;
  WB_TRY(s->kc.ensure_zeroed((size_t)NL * pool * d * 4, s->st));
  WB_TRY(s->vc.ensure_zeroed((size_t)NL * pool * d * 4, s->st));
  WB_TRY(s->tabs.ensure((size_t)2 * S * max_len * 4));
  s->lay = make_step_layout(S, s->W);
  WB_TRY(s->state.ensure((size_t)s->lay.total * 4));
  // step state and top-k results live in mapped pinned host memory: the prepare kernel pulls the
  // state over PCIe, the merge kernel pushes the k (id, log-prob) pairs -- no copy launches per step
  const size_t host_bytes = (size_t)s->lay.total * 4 + (size_t)S * TOPK_MAX * 8 + (size_t)S * 2 * 4;   // + chain flags
  if (s->host_bytes < host_bytes) {
    if (s->host_block) { (void)hipHostFree(s->host_block); s->host_block = nullptr; s->host_bytes = 0; }
    WB_HIP(hipHostMalloc((void**)&s->host_block, host_bytes, hipHostMallocMapped));
    s->host_bytes = host_bytes;
  }
  WB_HIP(hipHostGetDevicePointer((void**)&s->host_block_dev, s->host_block, 0));
  s->state_host = reinterpret_cast<int*>(s->host_block);
  s->topk_id_host = reinterpret_cast<int32_t*>(s->host_block + (size_t)s->lay.total * 4);
  s->topk_lp_host = reinterpret_cast<float*>(s->host_block + (size_t)s->lay.total * 4 + (size_t)S * TOPK_MAX * 4);
  s->chain_flags_off = (size_t)s->lay.total * 4 + (size_t)S * TOPK_MAX * 8;
  gemv_plan(d, 3 * d, &s->ks_qkv, &s->ksl_qkv);
  gemv_plan(d, d, &s->ks_o, &s->ksl_o);
  gemv_plan(d, 4 * d, &s->ks_1, &s->ksl_1);
  gemv_plan(4 * d, d, &s->ks_2, &s->ksl_2);
  s->ks_v = 1; s->ksl_v = d;                    // logits: whole rows per block (tile statistics need complete sums)
  s->ct_v = GV_CT_LOGITS;
  s->n_tiles_v = (V + s->ct_v - 1) / s->ct_v;
  // (+ 8 rows of slack: the fused kernels read whole MR-row tiles unconditionally, live or not)
  WB_TRY(s->x.ensure(((size_t)2 * S + 8) * d * 4));   // residual stream, ping-pong
  WB_TRY(s->h.ensure((size_t)S * d * 4));
  WB_TRY(s->att.ensure((size_t)S * d * 4));
  WB_TRY(s->hm.ensure((size_t)S * 4 * d * 4));
  // (batch mode's skinny GEMM, decode_batch.hip, splits K its own way: the plane buffers hold the larger count)
  s->sk_qkv = skinny_ksplit(d, 3 * d, KS_MAX, S); s->sk_o = skinny_ksplit(d, d, KS_MAX, S);
  s->sk_1 = skinny_ksplit(d, 4 * d, KS_MAX, S); s->sk_2 = skinny_ksplit(4 * d, d, KS_MAX, S);
  WB_TRY(s->Pqkv.ensure((size_t)std::max(s->ks_qkv, s->sk_qkv) * S * 3 * d * 4));
  WB_TRY(s->Po.ensure(((size_t)std::max(s->ks_o, s->sk_o) * S + 8) * d * 4));
  WB_TRY(s->Pq.ensure((size_t)std::max(s->ks_o, s->sk_o) * S * d * 4));
  WB_TRY(s->P1.ensure((size_t)std::max(s->ks_1, s->sk_1) * S * 4 * d * 4));
  WB_TRY(s->P2.ensure(((size_t)std::max(std::max(s->ks_2, s->sk_2), dec_mlp_fused_planes(d)) * S + 8) * d * 4));

  WB_TRY(s->Pa.ensure(((size_t)D.n_text_head * S + 8) * d * 4));
  WB_TRY(s->Pc.ensure(((size_t)D.n_text_head * S + 8) * d * 4));
  WB_TRY(s->carec.ensure(((size_t)D.n_text_head * std::max(1, s->n_chunks) * S + 8) * (d + 2) * 4));
  WB_TRY(s->ca.ensure((size_t)S * D.n_text_head * std::max(1, s->n_chunks) * CA_STRIDE * 4));
  WB_TRY(s->logits.ensure((size_t)S * V * 4));
  WB_TRY(s->tstats.ensure((size_t)S * s->n_tiles_v * TS_STRIDE * 4));
  WB_TRY(s->row_stats.ensure((size_t)S * 2 * 4));
  WB_TRY(s->lp_tmp.ensure((size_t)V * 4));
  s->decode_ready = true;
  return WB_OK;
}

}  // namespace wb

void wb_session::clear_graphs() {
  for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
  graphs.clear();
}

wb_session::~wb_session() {
  clear_graphs();
  if (host_block) (void)hipHostFree(host_block);
  if (guard_host) (void)hipHostFree(guard_host);
  if (pcm_stage) (void)hipHostFree(pcm_stage);
  if (ps_pin) (void)hipHostFree(ps_pin);
  if (ev_seg) (void)hipEventDestroy(ev_seg);
  if (st2) (void)hipStreamDestroy(st2);
  if (st) (void)hipStreamDestroy(st);
}

extern "C" {

int wb_session_begin(wb_model* m, const float* pcm, int64_t n_pcm, const int64_t* starts, const int64_t* lens,
                     int n_windows, int max_beams, int padding, wb_session** out) {
  WB_REQUIRE(m && pcm && starts && lens && out, WB_ERR_ARG, "wb_session_begin: null argument");
  wb::GpuTurn turn(m->device);
  wb_session* s = nullptr;
  WB_TRY(session_create(m, n_windows, max_beams, padding, &s));
  int rc = session_encode_pcm(s, pcm, n_pcm, starts, lens, false);
  if (rc != WB_OK) { wb_session_free(s); return rc; }
  *out = s;
  return WB_OK;
}

int wb_session_begin_mel(wb_model* m, const float* mel, const int32_t* T, int n_windows, int max_beams, int padding,
                         wb_session** out) {
  WB_REQUIRE(m && mel && T && out, WB_ERR_ARG, "wb_session_begin_mel: null argument");
  wb::GpuTurn turn(m->device);
  wb_session* s = nullptr;
  WB_TRY(session_create(m, n_windows, max_beams, padding, &s));
  const int clip = m->max_mel_frames() - padding;
  int maxT = 0;
  for (int w = 0; w < n_windows; w++) {
    if (T[w] < 1) { wb_session_free(s); set_error("window %d: empty mel", w); return WB_ERR_SHAPE; }
    s->T[w] = std::min(T[w], clip) + padding;   // transcribe.rs:171-177
    maxT = std::max(maxT, s->T[w]);
  }
  const int Ts = (maxT + 3) & ~3, NMEL = m->dims.n_mels;
  std::vector<float> host((size_t)n_windows * NMEL * Ts, 0.f);
  const float* src = mel;
  for (int w = 0; w < n_windows; w++) {
    const int keep = s->T[w] - padding;
    for (int r = 0; r < NMEL; r++) memcpy(&host[((size_t)w * NMEL + r) * Ts], src + (size_t)r * T[w], (size_t)keep * 4);
    src += (size_t)NMEL * T[w];
  }
  int rc = s->mel.ensure(host.size() * 4);
  if (rc == WB_OK && (hipMemcpyAsync(s->mel.p, host.data(), host.size() * 4, hipMemcpyHostToDevice, s->st) != hipSuccess ||
                      hipStreamSynchronize(s->st) != hipSuccess)) {
    set_error("mel upload failed");
    rc = WB_ERR_HIP;
  }
  if (rc == WB_OK) {
    MelBatch mb;
    mb.mel = s->mel.as<float>(); mb.win_stride = (int64_t)NMEL * Ts; mb.row_stride = Ts; mb.T = s->T;
    rc = session_finish_encode(s, mb);
  }
  if (rc != WB_OK) { wb_session_free(s); return rc; }
  *out = s;
  return WB_OK;
}

void wb_session_free(wb_session* s) {
  if (!s) return;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.find(s->model_uid);   // absent: the model was freed first -- s->m dangles and must not be touched
                                            // (a NEW model at the same address has another uid: no false match)
    if (it != g_pool.end()) {
      size_t parked = 0;
      for (const wb_session* q : it->second) parked += session_device_bytes(q);
      // keep the allocations (and captured graphs) for the next batch, within a byte budget
      if (sw::session_pool() && it->second.size() < POOL_MAX_SESSIONS && parked + session_device_bytes(s) <= POOL_MAX_BYTES) {
        it->second.push_back(s);
        return;
      }
    }
  }
  (void)hipSetDevice(s->device);
  delete s;
}

int wb_session_set_special_mask(wb_session* s, const uint8_t* is_special) {
  WB_REQUIRE(s && is_special, WB_ERR_ARG, "wb_session_set_special_mask: null argument");
  wb::GpuTurn turn(s->device);
  const int V = s->m->dims.n_vocab;
  WB_HIP(hipSetDevice(s->m->device));
  WB_TRY(s->mask.ensure((size_t)V * 4));
  // a pooled session that already holds this mask on the device (the usual case: one tokenizer per process) skips the
  // 200 KB upload and its synchronisation -- ~40 us of every wb_waveform_to_tokens call
  if (s->mask_dev_ptr == s->mask.p && (int)s->mask_host.size() == V && memcmp(s->mask_host.data(), is_special, (size_t)V) == 0) {
    s->has_mask = true;
    return WB_OK;
  }
  s->mask_host.clear(); s->mask_dev_ptr = nullptr;                       // void the cache key before the contents change
  std::vector<float> mk(V);
  for (int i = 0; i < V; i++) mk[i] = is_special[i] ? -INFINITY : 0.f;   // transcribe.rs:244
  // (on the session's own stream: a copy on the legacy stream fails while ANOTHER session of the process is capturing a
  // step graph -- "would make the legacy stream depend on a capturing blocking stream", profiles/r06_b_two_lanes.txt)
  WB_HIP(hipMemcpyAsync(s->mask.p, mk.data(), (size_t)V * 4, hipMemcpyHostToDevice, s->st));
  WB_HIP(hipStreamSynchronize(s->st));
  s->mask_host.assign(is_special, is_special + V); s->mask_dev_ptr = s->mask.p;
  s->has_mask = true;
  return WB_OK;
}

int wb_session_last_logprobs(wb_session* s, int slot, float* out) {
  WB_REQUIRE(s && out, WB_ERR_ARG, "wb_session_last_logprobs: null argument");
  WB_REQUIRE(s->last_had_logits && slot >= 0 && slot < s->prev_n, WB_ERR_STATE,
             "wb_session_last_logprobs: no logits for slot %d", slot);
  const int V = s->m->dims.n_vocab;
  wb::GpuTurn turn(s->device);
  WB_HIP(hipSetDevice(s->m->device));
  launch_dec_logprob_row(s->st, s->logits.as<float>() + (size_t)slot * V, 1, (int64_t)s->S * V, V,
                         s->mask.as<float>(), s->last_use_mask,
                         s->row_stats.as<float>() + 2 * slot, s->lp_tmp.as<float>());
  WB_HIP(hipMemcpyAsync(out, s->lp_tmp.p, (size_t)V * 4, hipMemcpyDeviceToHost, s->st));
  WB_HIP(hipStreamSynchronize(s->st));
  return WB_OK;
}

int wb_session_encoder_output(wb_session* s, int w, float* out, int32_t* C) {
  WB_REQUIRE(s && w >= 0 && w < s->W, WB_ERR_ARG, "wb_session_encoder_output: bad argument");
  const int d = s->m->dims.n_audio_state;
  if (C) *C = s->C[w];
  if (out) {
    wb::GpuTurn turn(s->device);
    WB_HIP(hipSetDevice(s->m->device));
    WB_HIP(hipMemcpyAsync(out, s->enc_out.as<float>() + (size_t)s->row0[w] * d, (size_t)s->C[w] * d * 4,
                          hipMemcpyDeviceToHost, s->st));
    WB_HIP(hipStreamSynchronize(s->st));
  }
  return WB_OK;
}

}  // extern "C"
