// Profiling: the timed regions of the stages (ScopedTimer) and the per-kernel-class accumulators of the tagged launches.
#include <mutex>

#include "session.h"

using namespace wb;

namespace wb {

Profile& profile() {
  static Profile p;
  return p;
}

ScopedTimer::ScopedTimer(hipStream_t s, int slot_) : st(s), slot(slot_), on(profile().on) {
  if (!on) return;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
  (void)hipEventRecord(a, st);
}
void ScopedTimer::stop() {
  if (on) (void)hipEventRecord(b, st);
}

// ---- per-kernel profiling --------------------------------------------------------------------------------
static const char* const g_kernel_names[KC_COUNT] = {
    "dec_prepare", "dec_attn_fused (LN + QKV + self-attention + out-proj)", "dec_cross_attn (LN + Wq + cross-attention)",
    "dec_gemv cross-attn out-proj", "dec_mlp_fused (LN + lin1 + GELU + lin2)", "dec_gemv logits (LN + E^T + tile stats)",
    "dec_topk_merge", "dec_gemv LN + QKV", "dec_self_attn", "dec_gemv self-attn out-proj", "dec_gemv LN + Wq",
    "dec_gemv LN + lin1", "dec_gemv GELU + lin2", "dec_cross_fused (LN + Wq + cross-attention + out-proj)",
    "batch: dec_resolve_ln (fold + LayerNorm)", "batch: split-K MFMA GEMM (decoder weight stream)",
    "batch: dec_self_attn (paged self-KV)", "batch: dec_cross_attn_stream (cached K/V stream)",
    "batch: dec_cross_attn chunked (cached K/V, beams)", "batch: dec_attn_combine", "batch: dec_gelu_fold",
    "batch: logits MFMA GEMM (E^T stream)", "batch: dec_topk_rows", "dec_persist (flag-chained decode steps)",
    "dec_beam_update (beam.rs bookkeeping on the device)", "dec_fold_ln_rows (final fold + LayerNorm, 9 - 16 rows)",
    "align_row_stats (cross-attention score max / sum)", "align_accumulate (weights + z-score + median + head mean)",
    "align_dtw (anti-diagonal DTW + backtrace)", "score_logits (LN rows x E^T -> per-split max / sum, target, probes)",
    "score_merge (splits -> lse, log-probs)", "dec_sample_update (Gumbel-max draw + row bookkeeping)",
    "dec_ts_update (timestamp rules + pick + row bookkeeping)",
    "dec_tsbeam_rows (timestamp rules + B + 1 candidates per row)", "dec_tsbeam_update (beam bookkeeping under the timestamp rules)",
    "prefill_store (prompt pass K / V -> paged self-KV cache, position tables)"};
struct PendingLaunch { hipEvent_t a, b; int cls; double bytes; };
static std::mutex g_prof_mu;
static std::vector<PendingLaunch> g_pending;
static KernelStat g_kstats[KC_COUNT];
static thread_local hipEvent_t tl_ev_a = nullptr, tl_ev_b = nullptr;

void prof_tag(int cls, double algo_bytes) {
  if (!profile().on) return;
  hipEvent_t a = nullptr, b = nullptr;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
  {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_pending.push_back(PendingLaunch{a, b, cls, algo_bytes});
  }
  tl_ev_a = a; tl_ev_b = b;
}
void prof_adjust_bytes(int cls, double delta) {
  if (!profile().on) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_kstats[cls].bytes += delta;
}
bool prof_take_events(hipEvent_t* start, hipEvent_t* stop) {
  if (!tl_ev_a) return false;
  *start = tl_ev_a; *stop = tl_ev_b;
  tl_ev_a = tl_ev_b = nullptr;
  return true;
}
void prof_collect() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (PendingLaunch& p : g_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      g_kstats[p.cls].calls++; g_kstats[p.cls].ms += ms; g_kstats[p.cls].bytes += p.bytes;
    }
    (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b);
  }
  g_pending.clear();
  (void)hipGetLastError();      // (a tag whose launch never happened fails its elapsed-time query: not a sticky error for later calls)
}
void ScopedTimer::collect() {
  if (!on) return;
  float ms = 0.f;
  if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) profile().ms[slot] += ms;
}
ScopedTimer::~ScopedTimer() {
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
}

}  // namespace wb

extern "C" {

int wb_profile_enable(int on) {
  profile().on = on != 0;
  return WB_OK;
}
int wb_profile_kernels(wb_kernel_stat* out, int cap, int reset) {
  WB_REQUIRE(out || cap == 0, WB_ERR_ARG, "wb_profile_kernels: null argument");
  prof_collect();
  int n = 0;
  for (int c = 0; c < KC_COUNT; c++) {
    if (g_kstats[c].calls == 0) continue;
    if (n < cap) {
      snprintf(out[n].name, sizeof(out[n].name), "%s", g_kernel_names[c]);
      out[n].calls = g_kstats[c].calls; out[n].total_ms = g_kstats[c].ms; out[n].algo_bytes = g_kstats[c].bytes;
    }
    n++;
  }
  if (reset)
    for (int c = 0; c < KC_COUNT; c++) g_kstats[c] = KernelStat();
  return n;
}
int wb_profile_read(double* out8, int reset) {
  WB_REQUIRE(out8, WB_ERR_ARG, "wb_profile_read: null argument");
  for (int i = 0; i < 8; i++) out8[i] = profile().ms[i];
  if (reset)
    for (int i = 0; i < 8; i++) profile().ms[i] = 0;
  return WB_OK;
}

}  // extern "C"
