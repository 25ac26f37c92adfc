// One decode step: the plan that picks its kernels (plan_step), their enqueue, the graph capture / replay around it
// (launch_step) and the host-driven step entry point (wb_session_step).
#include "decode_step.h"

#include <cstring>
#include <mutex>

#include "switches.h"

using namespace wb;

namespace wb {

// Range guard of the split-precision decoder GEMM (decode_batch.hip): called wherever a decode has just synchronised with
// the host.  The kernel raises the model's mapped flag word when a result is not finite (an activation outside fp16's
// range, |x| >= 65504: attention outputs and GELU hidden units are the only GEMM inputs that are not LayerNorm outputs).
// The call that observes it fails loudly, the model switches to the exact-f32 skinny kernel for good and this session's
// captured step graphs are dropped, so the caller's retry decodes with f32 GEMMs.  The flag word is this SESSION's
// (guard_host[1]): only the session whose rows were invalid fails; the others keep their (finite) results and drop their
// own graphs at their next look-up, where the graph signature carries the model's switch (launch_step).
int dec_split_check(wb_session* s) {
  wb_model* m = s->m;
  if (!s->guard_host || __atomic_load_n(&s->guard_host[1], __ATOMIC_ACQUIRE) == 0) return WB_OK;
  __atomic_store_n(&s->guard_host[1], 0, __ATOMIC_RELEASE);
  __atomic_store_n(&m->dec_split_off, 1, __ATOMIC_RELEASE);
  s->clear_graphs();
  WB_REQUIRE(false, WB_ERR_STATE, "a decoder activation left fp16's range under the split-precision decode GEMM: this call's "
             "rows are invalid; the model now uses the exact-f32 decoder GEMMs -- decode again");
  return WB_OK;
}

StepPlan plan_step(const wb_session* s, int live_rows, bool allow_16row_bucket) {
  const wb_dims& D = s->m->dims;
  const int d = D.n_text_state, H = D.n_text_head, S = s->S, n = live_rows;
  StepPlan p;
  p.use_graph = sw::graph() && !profile().on;
  // sublayer fusion (decode_fused.hip): self-attention block and MLP block are ONE launch each
  p.fuse_sub = sw::fuse_sub() && dec_fused_supported(d) && d == 64 * H;
  // the whole cross-attention sublayer (LN + Wq + attention over the window's cached K/V + Wo) as one launch per
  // (head, beam): 10.6 us against 9.5 + 5.9 us (+ a kernel boundary) for chunked cross-attention + out-projection GEMV
  // once the block keeps its head's whole K in flight (decode_fused.hip); WHISPER_HIP_FUSE_X=0 restores the chunked pair
  p.fuse_x = sw::fuse_x() && p.fuse_sub && s->maxC <= CROSS_FUSED_MAX_PASSES * CROSS_FUSED_MAX_C;
  // launch shape: bucketed so that the same captured graph serves every step of a decode.  9 - 16 live rows (the reference's
  // live setting: beam 5 over a 30 s chunk = 15 rows, transcribe.rs:232-233) stay on the fused sublayer kernels where those
  // exist (d <= 512): the attention / cross-attention blocks are per (head, row) anyway, the MLP block and the logits GEMV
  // run their 8-row tiles as two row groups -- 16 launches per step instead of batch mode's 54 (WHISPER_HIP_FUSE16=0: batch
  // mode).  The 16-row launch shape runs the fused kernels only: it needs both of them, and not the opt-in chunk records.
  p.g16 = allow_16row_bucket && sw::fuse16() && !sw::fuse_co() && p.fuse_sub && p.fuse_x && n > 8 && n <= 16 && S >= 9;
  p.n_launch = n <= 4 ? std::min(4, S) : n <= 8 ? std::min(8, S) : p.g16 ? std::min(16, S) : S;
  p.fuse_ln = p.n_launch <= 8 || p.g16;      // LayerNorm in the GEMV prologue (redundant per block) vs its own launch
  p.max_nb = s->max_beams <= 1 ? 1 : s->max_beams <= 2 ? 2 : s->max_beams <= 4 ? 4 : 8;
  if (p.fuse_ln) {
    // small models, exact-f32 weights, few enough blocks for one resident wave of them: the cross-attention blocks
    // project their own queries (decode.hip)
    p.fuse_q = sw::fuse_q() && cross_attn_can_fuse_q(d) && s->n_chunks * H * s->W <= 256;
    // ... or (older, opt-in) the chunked cross-attention blocks apply their head's rows of the out-projection
    // (opt-in: with 128-key chunks the MLP prologue has 6 H records per row to combine and loses what the launch saves)
    p.fuse_co = sw::fuse_co() && p.fuse_sub && p.fuse_q && H * s->n_chunks <= 48 && !p.fuse_x;
    p.ks_mlp = p.fuse_sub ? dec_mlp_fused_planes(d) : s->ks_2;
    // the persistent flag-chained kernel (decode_persist.hip): the small-batch fused path of exact-f32 models whose roles
    // fit one co-resident grid.  Default since it passed the graph-replayed chain of one launch per sublayer on MI355X
    // (14.76 vs 15.5 ms per 30 s of tiny.en audio, profiles/r03_c_ab_*); WHISPER_HIP_PERSIST=0 selects the chain.
    p.persist = sw::persist() && p.fuse_sub && p.fuse_x && dec_persist_supported(d, n, s->maxC);
  } else {
    // the skinny weight-stream GEMM (decode_batch.hip) for up to 64 rows of exact-f32 models: every weight row in flight
    // from the start.  WHISPER_HIP_BATCH_SKINNY=0 keeps the tiled GEMM.
    p.skinny = sw::batch_skinny() && p.n_launch <= 64 && s->sk_qkv > 0 && s->sk_o > 0 && s->sk_1 > 0 && s->sk_2 > 0;
    // one beam per window (greedy over many windows): one block per (head, window) streams the whole cached K/V and
    // writes the normalised head outputs -- no 128-key chunk partials, no combine launch (WHISPER_HIP_CROSS_STREAM=0:
    // the chunked kernel + combine)
    p.cross_stream = sw::cross_stream() && p.max_nb <= 1;
    // ... and where the head's slice of Wq is small next to the window's cached K/V (d <= 768: `small` and below) those
    // blocks fold the pending planes, normalise and project their own query first -- two launches less per layer.
    // Measured both ways (profiles/r03_j_*): small, 10 min +3 %; large-v2 (327 KB of Wq per block, 220 VGPRs)
    // 441x -> 433x, so d = 1024 / 1280 keep the launches.  WHISPER_HIP_CROSS_STREAM_FUSE=0 / 1 forces it off / on.
    const int mode = sw::cross_stream_fuse();
    p.stream_fused = p.cross_stream && cross_stream_can_fuse(d) && (mode < 0 ? d <= 768 : mode == 1);
    p.kq = p.skinny ? s->sk_qkv : s->ks_qkv; p.ko = p.skinny ? s->sk_o : s->ks_o;
    p.k1 = p.skinny ? s->sk_1 : s->ks_1; p.k2 = p.skinny ? s->sk_2 : s->ks_2;
  }
  return p;
}

namespace {
// What the pieces of one step's enqueue share: the session's buffers as the kernels see them, the residual stream's
// ping-pong index, and the byte counts of the tagged launches.
struct StepCtx {
  wb_session* s; const StepPlan& p; const StepCall& c;
  wb_model* m; hipStream_t st;
  int d, H, NL, V, S, n;
  const int* dst; int* tabs;
  float* xb[2]; int xi = 0;                       // xb[xi] holds the current residual stream
  float *h, *att;
  size_t pool;
  int ldkv; const int* win_row0; const int* win_C;
  // algorithmic bytes of the tagged launches (profiling): the weights a launch streams + the cached K/V it reads
  double wsz = 4.0, dd, ckv_bytes = 0, self_kv_bytes;
  bool dec_split;

  StepCtx(wb_session* s_, const StepPlan& p_, const StepCall& c_) : s(s_), p(p_), c(c_), m(s_->m), st(s_->st) {
    const wb_dims& D = m->dims;
    d = D.n_text_state; H = D.n_text_head; NL = D.n_text_layer; V = D.n_vocab; S = s->S; n = p.n_launch;
    dst = s->state.as<int>(); tabs = s->tabs.as<int>();
    xb[0] = s->x.as<float>(); xb[1] = s->x.as<float>() + (size_t)S * d;
    h = s->h.as<float>(); att = s->att.as<float>();
    pool = (size_t)s->Lmax * S;
    ldkv = 2 * d;
    win_row0 = s->win_meta.as<int>(); win_C = win_row0 + s->W;
    dd = (double)d * d;
    for (int cw : s->C) ckv_bytes += 8.0 * cw * d;                    // K and V rows of one layer, f32
    self_kv_bytes = 8.0 * (double)n * (s->step + s->prof_step_off + 1) * d;
    dec_split = m->dec_split_active();
  }
  // cached cross K|V: layer-major, [layer][packed encoder row][2d] (session_finish_encode) -- layer l's rows start at ckv_of(l)
  const float* ckv_of(int l) const { return s->ckv.as<float>() + (size_t)l * s->enc_rows * 2 * d; }
  float* kc_of(int l) const { return s->kc.as<float>() + (size_t)l * pool * d; }
  float* vc_of(int l) const { return s->vc.as<float>() + (size_t)l * pool * d; }

  GemvArgs gemv(const LinearW& w, int ks, int ksl, int pro, const float* src, int ld_src, float* P) const {
    GemvArgs a;
    a.W = w.w; a.ldw = w.n; a.K = w.k; a.N = w.n; a.KS = ks; a.KSL = ksl; a.pro = pro; a.src = src; a.ld_src = ld_src;
    a.P = P; a.st = dst; a.S = S;
    return a;
  }
  // y = W . LN(x + pending): folds the pending sublayer output into the residual stream (ping-pong),
  // normalises, multiplies -- in one launch when few beams are live
  void ln_gemv(GemvArgs a, const float* pend, int ks_pend, const float* pbias, const LayerNormW& ln, bool stats) {
    a.ln_g = ln.g; a.ln_b = ln.b; a.ln_eps = ln.eps; a.ln_inside = m->ln_eps_inside_sqrt;
    a.pro = PRO_LN; a.src = xb[xi]; a.ld_src = d; a.pend = pend; a.KSp = ks_pend; a.pbias = pbias; a.x_out = xb[xi ^ 1];
    launch_dec_gemv(st, a, n, stats);
    xi ^= 1;
  }
  // batch mode: fold the pending planes into the residual stream and normalise, in a launch of its own
  void resolve(const float* pend, int ks_pend, const float* pbias, const LayerNormW& ln) {
    prof_tag(KC_B_RESOLVE_LN, 4.0 * n * d * (ks_pend + 3));
    launch_dec_resolve_ln(st, dst, n, xb[xi], xb[xi ^ 1], pend, ks_pend, S, pbias, d, ln, m->ln_eps_inside_sqrt, h);
    xi ^= 1;
  }
  // batch mode: P[ks planes] = A . w, split-K, each weight streamed once -- the skinny weight-stream GEMM or the tiled one
  int proj(const LinearW& w, int ks, const float* A, float* P) const {
    prof_tag(KC_B_GEMM, wsz * (double)w.k * w.n + 4.0 * n * ((double)w.k + (double)ks * w.n));
    if (p.skinny) {
      SkinnyArgs g;
      g.A = A; g.lda = w.k; g.B = w.w; g.ldb = w.n; g.M = n; g.N = w.n; g.K = w.k; g.ksplit = ks;
      g.P = P; g.plane = S * w.n;
      if (dec_split && w.th && w.tl) { g.Bh = w.th; g.Bl = w.tl; g.range_flag = s->guard_dev + 1; g.st = dst; }   // 16-bit matrix path, f32-grade
      WB_REQUIRE(launch_dec_skinny_gemm(st, g) == 0, WB_ERR_SHAPE, "skinny gemm: unsupported shape M=%d N=%d K=%d ks=%d", n,
                 w.n, w.k, ks);
      return WB_OK;
    }
    GemmArgs g;
    g.A = A; g.lda = w.k; g.B = w.w; g.ldb = w.n; g.C = P; g.ldc = w.n; g.M = n; g.N = w.n; g.K = w.k;
    g.ksplit = ks; g.c_split_stride = (int64_t)S * w.n;
    return gemm_dispatch(m, st, g, w.k);
  }
};
}  // namespace

// ---- batch mode (more than 8 live beams; more than 16 on the fused models): rows are many enough for the matrix cores ----
// LayerNorm in its own launch, split-K exact-f32 MFMA GEMMs streaming each weight once into the
// same partial-sum planes the small-batch consumers fold.  Leaves the last MLP's planes (P2, k2) pending.
static int enqueue_layers_batch(StepCtx& c) {
  wb_session* s = c.s; wb_model* m = c.m; const StepPlan& p = c.p;
  hipStream_t st = c.st;
  const int d = c.d, H = c.H, S = c.S, n = c.n;
  const StepLayout& L = s->lay;
  float *h = c.h, *att = c.att, *hm = s->hm.as<float>();
  const int kq = p.kq, ko = p.ko, k1 = p.k1, k2 = p.k2;
  const float* pend = nullptr; int ks_pend = 0; const float* pbias = nullptr;
  for (int l = 0; l < c.NL; l++) {
    const DecBlockW& b = m->dec[l];
    c.resolve(pend, ks_pend, pbias, b.ln1);
    WB_TRY(c.proj(b.qkv, kq, h, s->Pqkv.as<float>()));
    prof_tag(KC_B_SELF_ATTN, c.self_kv_bytes + 4.0 * n * 3 * d * kq);
    s->prof_cls_self = KC_B_SELF_ATTN;
    launch_dec_self_attn(st, c.dst, L, n, H, s->Pqkv.as<float>(), kq, b.qkv.b, d, c.kc_of(l), c.vc_of(l), c.tabs,
                         s->Lmax, m->qk_scale, att);
    WB_TRY(c.proj(b.out, ko, att, s->Po.as<float>()));
    if (p.stream_fused) {
      // fold + cross_attn_ln + Wq inside the streaming blocks: two launches less per layer
      CaStreamFuse fz;
      fz.x_in = c.xb[c.xi]; fz.x_out = c.xb[c.xi ^ 1]; fz.pend = s->Po.as<float>(); fz.KSp = ko; fz.pbias = b.out.b;
      fz.ln_g = b.ln2.g; fz.ln_b = b.ln2.b; fz.ln_eps = b.ln2.eps; fz.ln_inside = m->ln_eps_inside_sqrt; fz.Wq = b.cq.w;
      prof_tag(KC_B_CROSS_STREAM, c.ckv_bytes + 4.0 * c.dd + 4.0 * n * d * (ko + 2));
      s->prof_cls_cross = KC_B_CROSS_STREAM;
      launch_dec_cross_attn_stream_fused(st, c.dst, L, s->W, H, b.cq.b, d, c.ckv_of(l), c.ldkv, 0, c.win_row0,
                                         c.win_C, m->qk_scale, att, fz);
      c.xi ^= 1;
    } else {
      c.resolve(s->Po.as<float>(), ko, b.out.b, b.ln2);
      WB_TRY(c.proj(b.cq, ko, h, s->Pq.as<float>()));
      if (p.cross_stream) {
        prof_tag(KC_B_CROSS_STREAM, c.ckv_bytes + 4.0 * n * d * (ko + 1));
        s->prof_cls_cross = KC_B_CROSS_STREAM;
        launch_dec_cross_attn_stream(st, c.dst, L, s->W, H, s->Pq.as<float>(), ko, b.cq.b, d, c.ckv_of(l), c.ldkv,
                                     0, c.win_row0, c.win_C, m->qk_scale, att);
      } else {
        prof_tag(KC_B_CROSS_CHUNK, c.ckv_bytes + 4.0 * n * d * ko);
        s->prof_cls_cross = KC_B_CROSS_CHUNK;
        launch_dec_cross_attn(st, c.dst, L, s->W, H, s->n_chunks, s->Pq.as<float>(), ko, b.cq.b, d, c.ckv_of(l),
                              c.ldkv, 0, c.win_row0, c.win_C, m->qk_scale, s->ca.as<float>(), p.max_nb);
        prof_tag(KC_B_COMBINE, 4.0 * n * H * s->n_chunks * CA_STRIDE);
        launch_dec_attn_combine(st, c.dst, n, s->ca.as<float>(), H, s->n_chunks, att);
      }
    }
    WB_TRY(c.proj(b.cout, ko, att, s->Po.as<float>()));
    c.resolve(s->Po.as<float>(), ko, b.cout.b, b.ln3);
    WB_TRY(c.proj(b.mlp1, k1, h, s->P1.as<float>()));
    prof_tag(KC_B_GELU_FOLD, 4.0 * n * 4 * d * (k1 + 1));
    launch_dec_gelu_fold(st, c.dst, n, s->P1.as<float>(), k1, S, 4 * d, b.mlp1.b, hm);
    WB_TRY(c.proj(b.mlp2, k2, hm, s->P2.as<float>()));
    pend = s->P2.as<float>(); ks_pend = k2; pbias = b.mlp2.b;
  }
  return WB_OK;
}

// ---- small batch: fused sublayer kernels, or one GEMV per matrix with the LayerNorm in its prologue ----
// Leaves the last MLP's planes (P2, ks_mlp) pending.
static int enqueue_layers_small(StepCtx& c) {
  wb_session* s = c.s; wb_model* m = c.m; const StepPlan& p = c.p;
  hipStream_t st = c.st;
  const int d = c.d, H = c.H, S = c.S, n = c.n;
  const StepLayout& L = s->lay;
  const double wsz = c.wsz, dd = c.dd;
  float* att = c.att;
  for (int l = 0; l < c.NL; l++) {   // ResidualDecoderAttentionBlock::forward, mod.rs:345-350
    const DecBlockW& b = m->dec[l];
    const float* pend_a = l == 0 ? nullptr : s->P2.as<float>();
    const int ks_a = l == 0 ? 0 : p.ks_mlp;
    const float* pb_a = l == 0 ? nullptr : m->dec[l - 1].mlp2.b;
    const float* att_planes; int att_ks;                     // what the cross-attention prologue folds
    if (p.fuse_sub) {
      AttnFusedArgs fa;
      fa.st = c.dst; fa.lay = L; fa.S = S; fa.d = d; fa.n_head = H;
      fa.x_in = c.xb[c.xi]; fa.pend = pend_a; fa.KSp = ks_a; fa.pbias = pb_a; fa.x_out = c.xb[c.xi ^ 1];
      fa.ln_g = b.ln1.g; fa.ln_b = b.ln1.b; fa.ln_eps = b.ln1.eps; fa.ln_inside = m->ln_eps_inside_sqrt;
      fa.Wqkv = b.qkv.w; fa.ldqkv = b.qkv.n; fa.bqkv = b.qkv.b; fa.scale = m->qk_scale;
      fa.Kc = c.kc_of(l); fa.Vc = c.vc_of(l);
      fa.tabs = c.tabs; fa.Lmax = s->Lmax; fa.Wo = b.out.w; fa.P = s->Pa.as<float>();
      prof_tag(KC_ATTN_FUSED, 4.0 * dd * 4 + c.self_kv_bytes);
      s->prof_cls_self = KC_ATTN_FUSED;
      launch_dec_attn_fused(st, fa, n);
      c.xi ^= 1;
      att_planes = s->Pa.as<float>(); att_ks = H;
    } else {
      prof_tag(KC_GEMV_LN_QKV, wsz * dd * 3);
      c.ln_gemv(c.gemv(b.qkv, s->ks_qkv, s->ksl_qkv, PRO_PLAIN, nullptr, d, s->Pqkv.as<float>()), pend_a, ks_a, pb_a, b.ln1, false);
      prof_tag(KC_SELF_ATTN, c.self_kv_bytes);
      s->prof_cls_self = KC_SELF_ATTN;
      launch_dec_self_attn(st, c.dst, L, n, H, s->Pqkv.as<float>(), s->ks_qkv, b.qkv.b, d, c.kc_of(l), c.vc_of(l), c.tabs,
                           s->Lmax, m->qk_scale, att);
      prof_tag(KC_GEMV_OUT, wsz * dd);
      launch_dec_gemv(st, c.gemv(b.out, s->ks_o, s->ksl_o, PRO_PLAIN, att, d, s->Po.as<float>()), n, false);
      att_planes = s->Po.as<float>(); att_ks = s->ks_o;
    }
    if (p.fuse_x) {
      CrossFusedArgs ca;
      ca.st = c.dst; ca.lay = L; ca.S = S; ca.d = d; ca.n_head = H;
      ca.x_in = c.xb[c.xi]; ca.pend = att_planes; ca.KSp = att_ks; ca.pbias = b.out.b; ca.x_out = c.xb[c.xi ^ 1];
      ca.ln_g = b.ln2.g; ca.ln_b = b.ln2.b; ca.ln_eps = b.ln2.eps; ca.ln_inside = m->ln_eps_inside_sqrt;
      ca.Wq = b.cq.w; ca.bq = b.cq.b; ca.scale = m->qk_scale;
      ca.ckv = c.ckv_of(l); ca.ldkv = c.ldkv; ca.koff = 0; ca.win_row0 = c.win_row0; ca.win_C = c.win_C;
      ca.Wo = b.cout.w; ca.P = s->Pc.as<float>();
      ca.n_pass = s->maxC > CROSS_FUSED_MAX_C ? 2 : 1;
      prof_tag(KC_CROSS_FUSED, c.ckv_bytes + 4.0 * dd * 2);
      s->prof_cls_cross = KC_CROSS_FUSED;
      launch_dec_cross_fused(st, ca, n);
      c.xi ^= 1;
    } else if (p.fuse_q) {
      // cross_attn_ln + the query projection inside the cross-attention blocks (one launch less per layer)
      CaFuse fz;
      fz.x_in = c.xb[c.xi]; fz.pend = att_planes; fz.KSp = att_ks; fz.pbias = b.out.b; fz.x_out = c.xb[c.xi ^ 1];
      fz.ln_g = b.ln2.g; fz.ln_b = b.ln2.b; fz.ln_eps = b.ln2.eps; fz.ln_inside = m->ln_eps_inside_sqrt;
      fz.Wq = b.cq.w;
      if (p.fuse_co) { fz.Wo = b.cout.w; fz.rec = s->carec.as<float>(); }
      prof_tag(KC_CROSS_ATTN, c.ckv_bytes + 4.0 * dd * (p.fuse_co ? 2 : 1));
      s->prof_cls_cross = KC_CROSS_ATTN;
      launch_dec_cross_attn(st, c.dst, L, s->W, H, s->n_chunks, nullptr, 0, b.cq.b, d, c.ckv_of(l), c.ldkv,
                            0, c.win_row0, c.win_C, m->qk_scale, s->ca.as<float>(), p.max_nb, &fz);
      c.xi ^= 1;
    } else {
      prof_tag(KC_GEMV_LN_CQ, wsz * dd);
      c.ln_gemv(c.gemv(b.cq, s->ks_o, s->ksl_o, PRO_PLAIN, nullptr, d, s->Pq.as<float>()), att_planes, att_ks, b.out.b, b.ln2,
                false);
      prof_tag(KC_CROSS_ATTN, c.ckv_bytes);
      s->prof_cls_cross = KC_CROSS_ATTN;
      launch_dec_cross_attn(st, c.dst, L, s->W, H, s->n_chunks, s->Pq.as<float>(), s->ks_o, b.cq.b, d,
                            c.ckv_of(l), c.ldkv, 0, c.win_row0, c.win_C, m->qk_scale, s->ca.as<float>(), p.max_nb);
    }
    if (!p.fuse_co && !p.fuse_x) {
      GemvArgs a = c.gemv(b.cout, s->ks_o, s->ksl_o, PRO_ATTN, s->ca.as<float>(), 0, s->Po.as<float>());
      a.n_head = H; a.n_chunks = s->n_chunks;
      prof_tag(KC_GEMV_COUT, wsz * dd);
      launch_dec_gemv(st, a, n, false);
    }
    if (p.fuse_sub) {
      MlpFusedArgs ma;
      ma.st = c.dst; ma.S = S; ma.d = d;
      ma.x_in = c.xb[c.xi]; ma.pend = s->Po.as<float>(); ma.KSp = s->ks_o; ma.pbias = b.cout.b; ma.x_out = c.xb[c.xi ^ 1];
      if (p.fuse_x) { ma.pend = s->Pc.as<float>(); ma.KSp = H; }
      else if (p.fuse_co) {   // the cross-attention blocks applied Wo themselves: fold their chunk records
        ma.pend = s->carec.as<float>(); ma.KSp = H * s->n_chunks; ma.n_head = H; ma.n_chunks = s->n_chunks;
      }
      ma.ln_g = b.ln3.g; ma.ln_b = b.ln3.b; ma.ln_eps = b.ln3.eps; ma.ln_inside = m->ln_eps_inside_sqrt;
      ma.W1 = b.mlp1.w; ma.ld1 = b.mlp1.n; ma.b1 = b.mlp1.b; ma.W2 = b.mlp2.w; ma.P = s->P2.as<float>();
      prof_tag(KC_MLP_FUSED, 4.0 * dd * 8);
      launch_dec_mlp_fused(st, ma, n);
      c.xi ^= 1;
    } else {
      prof_tag(KC_GEMV_LN_MLP1, wsz * dd * 4);
      c.ln_gemv(c.gemv(b.mlp1, s->ks_1, s->ksl_1, PRO_PLAIN, nullptr, d, s->P1.as<float>()), s->Po.as<float>(), s->ks_o,
                b.cout.b, b.ln3, false);
      GemvArgs a = c.gemv(b.mlp2, s->ks_2, s->ksl_2, PRO_GELU, s->P1.as<float>(), 4 * d, s->P2.as<float>());
      a.pbias = b.mlp1.b; a.KSp = s->ks_1;
      prof_tag(KC_GEMV_MLP2, wsz * dd * 4);
      launch_dec_gemv(st, a, n, false);
    }
  }
  return WB_OK;
}

// logits = ln(x + last MLP) . token_embedding^T (mod.rs:155-156), last position only, + mask; the k best per row; behind
// them the beam bookkeeping of a device-chained beam step; and, when this step is timed, the collect of its tagged launches.
static int enqueue_logits_tail(StepCtx& c, bool timed, bool merge_prepares, int* gctl) {
  wb_session* s = c.s; wb_model* m = c.m; const StepPlan& p = c.p; const StepCall& call = c.c;
  hipStream_t st = c.st;
  const int d = c.d, V = c.V, S = c.S, n = c.n, k = call.k;
  const StepLayout& L = s->lay;
  const BeamStepIO* bio = call.bio;
  const SampleStepIO* sio = call.sio;
  const TsStepIO* tio = call.tio;
  const TsBeamStepIO* tbio = call.tbio;
  int32_t* out_id_dev = bio ? bio->topk_id : sio ? sio->topk_id : tio ? tio->topk_id : tbio ? tbio->topk_id : reinterpret_cast<int32_t*>(s->host_block_dev + (size_t)L.total * 4);
  float* out_lp_dev = bio ? bio->topk_lp : sio ? sio->topk_lp : tio ? tio->topk_lp : tbio ? tbio->topk_lp
                          : reinterpret_cast<float*>(s->host_block_dev + (size_t)L.total * 4 + (size_t)S * TOPK_MAX * 4);
  const float* pend = s->P2.as<float>(); const float* pbias = m->dec[c.NL - 1].mlp2.b;   // what the last layer left pending
  if (!p.fuse_ln) c.resolve(pend, p.k2, pbias, m->ln_dec);
  ScopedTimer tm_logits(st, 6);
  if (!p.fuse_ln) {
    GemmArgs g;
    g.A = c.h; g.lda = d; g.B = m->tok_emb_t; g.ldb = m->vocab_ld; g.C = s->logits.as<float>(); g.ldc = V;
    g.M = n; g.N = V; g.K = d;
    prof_tag(KC_B_LOGITS_GEMM, c.wsz * (double)V * d + 4.0 * n * ((double)d + V));
    WB_TRY(gemm_dispatch(m, st, g, d));
    tm_logits.stop();
    prof_tag(KC_B_TOPK_ROWS, 4.0 * (double)n * V);
    launch_dec_topk_rows(st, s->state.as<int>(), n, s->logits.as<float>(), V, s->mask.as<float>(), call.use_mask, k, out_id_dev,
                         out_lp_dev, s->row_stats.as<float>(), L, gctl, s->gtok.as<int>(), s->Lmax, call.eot);
  } else {
    // + tile statistics: the merge kernel picks the k best from them
    GemvArgs a;
    a.W = m->tok_emb_t; a.ldw = m->vocab_ld; a.K = d; a.N = V; a.KS = 1; a.KSL = d;
    a.P = s->logits.as<float>(); a.st = c.dst; a.S = S;
    a.mask = s->mask.as<float>(); a.use_mask = call.use_mask; a.topk = k; a.tstats = s->tstats.as<float>(); a.ct = s->ct_v;
    a.h_tmp = c.h;                          // (9 - 16 rows: the fold + LayerNorm runs once, in its own launch, into this buffer)
    if (dec_logits_two_launches(a, n)) prof_tag(KC_FOLD_LN_ROWS, 4.0 * n * d * (p.ks_mlp + 3));   // (the product launch tags itself)
    else prof_tag(KC_LOGITS, c.wsz * (double)V * d + 4.0 * ((double)n * d + (double)n * V));
    c.ln_gemv(a, pend, p.ks_mlp, pbias, m->ln_dec, true);
    tm_logits.stop();
    NextPrep nx;
    if (merge_prepares) { nx.x = c.xb[0]; nx.E = m->tok_emb; nx.pos = m->dec_pos; nx.tabs = c.tabs; nx.d = d; }
    if (call.chained) nx.hflags = reinterpret_cast<int*>(s->host_block_dev + s->chain_flags_off);
    prof_tag(KC_TOPK_MERGE, 4.0 * n * s->n_tiles_v * TS_STRIDE);
    launch_dec_topk_merge(st, s->state.as<int>(), n, s->tstats.as<float>(), s->n_tiles_v, k, out_id_dev, out_lp_dev,
                          s->row_stats.as<float>(), L, gctl, s->gtok.as<int>(), s->Lmax, call.eot, nx);
  }
  if (bio) { prof_tag(KC_BEAM_UPDATE, 8.0 * n * k); launch_dec_beam_update(st, bio->upd); }
  if (sio) {   // the draw reads the row's logits (and the mask) once
    SampleChainArgs u = sio->upd;
    u.use_mask = call.use_mask;
    prof_tag(KC_SAMPLE_UPDATE, (call.use_mask ? 8.0 : 4.0) * (double)n * V);
    launch_dec_sample_update(st, u, n);
  }
  if (tio) {   // the rules read the row's logits and its suppress bytes once
    prof_tag(KC_TS_UPDATE, 5.0 * (double)n * V);
    launch_dec_ts_update(st, tio->upd, n);
  }
  if (tbio) {  // the rows read their logits twice (the second pass from L2); the bookkeeping reads the candidates
    prof_tag(KC_TSBEAM_ROWS, 9.0 * (double)n * V);
    launch_dec_tsbeam_rows(st, tbio->rows, n);
    prof_tag(KC_TSBEAM_UPDATE, 12.0 * n * TOPK_MAX);
    launch_dec_tsbeam_update(st, tbio->upd);
  }
  if (timed && tm_logits.on) {
    WB_HIP(hipStreamSynchronize(st));
    tm_logits.collect();
    prof_collect();
    profile().ms[7] += 1;
  }
  return WB_OK;
}

// Enqueue the kernels of one decode step on `st`.  Everything that changes from step to step (token
// ids, parents, lengths, the live-beam count, table parity) is read by the kernels from the step
// state, so for a given (row bucket, k, mask, fuse) the launch sequence is identical every step and
// can be captured once into a hipGraph and replayed.
static int enqueue_step(wb_session* s, const StepPlan& p, const StepCall& call, bool timed) {
  StepCtx c(s, p, call);
  const BeamStepIO* bio = call.bio;
  const int* hst = bio ? bio->state_src : reinterpret_cast<const int*>(s->host_block_dev);   // mapped view of state_host
  int* gctl = call.chained ? s->gctl.as<int>() : nullptr;
  // chained small-batch steps: the previous step's merge kernel already prepared this one (the chain's
  // first step is prepared by session_greedy_chain)
  const bool merge_prepares = call.chained && p.fuse_ln;
  // (device-chained beam search / sampling: the bookkeeping launch behind the previous step prepared this one)
  if (!merge_prepares && !bio && !call.sio && !call.tio && !call.tbio) {
    prof_tag(KC_PREPARE, 8.0 * c.n * c.d);
    launch_dec_prepare(c.st, hst, s->state.as<int>(), s->lay, c.n, c.tabs, s->Lmax, s->m->tok_emb, s->m->dec_pos, c.d, c.xb[0], gctl);
  }
  WB_TRY(p.fuse_ln ? enqueue_layers_small(c) : enqueue_layers_batch(c));
  if (call.k > 0) WB_TRY(enqueue_logits_tail(c, timed, merge_prepares, gctl));
  return WB_OK;
}

int launch_step(wb_session* s, const StepPlan& plan, const StepCall& call) {
  wb_model* m = s->m;
  hipStream_t st = s->st;
  const int reps = call.reps, eot = call.eot;
  if (!plan.use_graph) {
    for (int i = 0; i < reps; i++) {
      WB_TRY(enqueue_step(s, plan, call, true));
      if (call.chained || call.bio || call.sio || call.tio || call.tbio) s->prof_step_off++;
    }
    return WB_OK;
  }
  // graphs bake in buffer addresses and launch geometry: drop them if anything moved since capture
  uint64_t sig = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { sig = (sig ^ v) * 1099511628211ull; };
  for (const wb::DevMem* b : {&s->kc, &s->vc, &s->tabs, &s->state, &s->x, &s->h, &s->att, &s->Pqkv, &s->Po, &s->Pq,
                              &s->P1, &s->P2, &s->Pa, &s->Pc, &s->carec, &s->ca, &s->logits, &s->tstats, &s->row_stats, &s->mask, &s->ckv,
                              &s->win_meta, &s->gctl, &s->gtok, &s->hm, &s->bc_ctl, &s->bc_topk})
    mix((uint64_t)(uintptr_t)b->p);
  mix((uint64_t)(uintptr_t)s->host_block_dev);
  // (enc_rows: the layer-major cross-K/V cache puts layer l at ckv + l * enc_rows * 2d -- ckv_of -- so the per-layer pointers a
  // graph holds move with the batch's packed encoder rows even when no buffer does; maxC: picks the cross-attention kernel
  // and its pass count (enqueue_step);
  // dec_split_active: another session's trip switched the model's decoder GEMM under these graphs)
  for (int v : {s->S, s->W, s->Lmax, s->n_chunks, s->max_beams, m->ln_eps_inside_sqrt, eot, (int)m->dec_split_active(), s->enc_rows, s->maxC})
    mix((uint64_t)(int64_t)v);
  mix(m->uid);
  if (sig != s->buf_sig) { s->clear_graphs(); s->buf_sig = sig; }
  // (reps > 1: device-chained steps read their position from the control block, so one graph can hold
  // several consecutive steps and the host launches once per run)
  // (a beam-chain graph also bakes in the search's constants -- beam size = k, eot via the signature above, max_depth and the
  // first step's position via the control block layout: session_beam_chain drops the graphs when those change)
  // (the rest of the plan follows from n_launch, fuse_ln and what the signature above carries: the model, S, W, max_beams,
  // n_chunks, maxC -- and the process's switches)
  // (a sampling-chain graph bakes in its control block and max_depth: session_sample_chain drops ITS graphs when those change;
  // a timestamp-chain graph likewise, and its suppress buffers: session_ts_chain; so session_tsbeam_chain for its own)
  const uint64_t key = ((uint64_t)reps << 48) | ((uint64_t)plan.n_launch << 32) | ((uint64_t)call.k << 8) | (call.sio ? GRAPH_KEY_SAMPLE : 0u) |
                       (call.tio ? GRAPH_KEY_TS : 0u) | (call.tbio ? GRAPH_KEY_TSBEAM : 0u) |
                       (call.bio ? 8u : 0u) | (call.chained ? 4u : 0u) | ((uint64_t)call.use_mask << 1) | (plan.fuse_ln ? 1u : 0u);
  auto it = s->graphs.find(key);
  if (it == s->graphs.end()) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    static std::mutex capture_mu;                      // captures are rare; keep them off each other's toes
    std::lock_guard<std::mutex> lk(capture_mu);
    WB_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    int rc = WB_OK;
    for (int i = 0; i < reps && rc == WB_OK; i++) rc = enqueue_step(s, plan, call, false);
    hipError_t e = hipStreamEndCapture(st, &g);
    WB_TRY(rc);
    WB_HIP(e);
    WB_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    it = s->graphs.emplace(key, ge).first;
    s->n_captures++;
  }
  WB_HIP(hipGraphLaunch(it->second, st));
  return WB_OK;
}

}  // namespace wb

extern "C" {

int wb_session_step(wb_session* s, const int32_t* new_tokens, const int32_t* parent, const int32_t* window, int n,
                    int apply_special_mask, int k, int32_t* top_ids, float* top_logprobs) {
  WB_REQUIRE(s && new_tokens && parent && window, WB_ERR_ARG, "wb_session_step: null argument");
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int V = D.n_vocab, S = s->S;
  wb::GpuTurn turn(s->device);
  WB_HIP(hipSetDevice(m->device));
  if (!s->decode_ready) WB_TRY(session_reserve(s, D.n_text_ctx));
  WB_REQUIRE(n >= 1 && n <= S, WB_ERR_ARG, "wb_session_step: n = %d outside [1, %d]", n, S);
  WB_REQUIRE(k >= 0 && k <= TOPK_MAX && (k == 0 || (top_ids && top_logprobs)), WB_ERR_ARG, "wb_session_step: bad k");
  WB_REQUIRE(!apply_special_mask || s->has_mask, WB_ERR_STATE, "wb_session_step: special mask not set");
  WB_REQUIRE(s->step < s->Lmax, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->step + 1, s->Lmax);
  const StepLayout& L = s->lay;
  int* hs = s->state_host;
  memset(hs, 0, (size_t)L.total * 4);
  hs[ST_N] = n; hs[ST_STEP] = s->step;
  std::vector<int> len(n);
  for (int i = 0; i < n; i++) {
    WB_REQUIRE(new_tokens[i] >= 0 && new_tokens[i] < V, WB_ERR_ARG, "token id %d out of range [0,%d)", new_tokens[i], V);
    WB_REQUIRE(window[i] >= 0 && window[i] < s->W, WB_ERR_ARG, "beam %d: window %d out of range", i, window[i]);
    if (parent[i] < 0) {
      len[i] = 1;
    } else {
      WB_REQUIRE(parent[i] < s->prev_n, WB_ERR_ARG, "beam %d: parent %d is not a beam of the previous step", i, parent[i]);
      WB_REQUIRE(s->prev_win[parent[i]] == window[i], WB_ERR_ARG, "beam %d: parent belongs to another window", i);
      len[i] = s->prev_len[parent[i]] + 1;
    }
    WB_REQUIRE(len[i] <= s->Lmax, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", len[i], s->Lmax);   // mod.rs:134-139
    hs[L.tok + i] = new_tokens[i]; hs[L.parent + i] = parent[i]; hs[L.len + i] = len[i]; hs[L.win + i] = window[i];
    int& nb = hs[L.win_nb + window[i]];
    WB_REQUIRE(nb < s->max_beams, WB_ERR_ARG, "window %d has more than max_beams = %d live beams", window[i], s->max_beams);
    hs[L.win_slots + window[i] * MAX_BEAMS + nb] = i;
    nb++;
  }
  const StepPlan plan = plan_step(s, n, true);
  const int use_mask = apply_special_mask ? 1 : 0;
  hipStream_t st = s->st;
  ScopedTimer tm_step(st, 3);
  StepCall call;
  call.k = k; call.use_mask = use_mask;
  WB_TRY(launch_step(s, plan, call));
  tm_step.stop();
  WB_HIP(hipStreamSynchronize(st));   // results land in mapped host memory; state_host is reused by the next step
  WB_TRY(dec_split_check(s));
  s->last_had_logits = 0;
  if (k > 0) {
    for (int i = 0; i < n; i++)
      for (int j = 0; j < k; j++) {
        top_ids[i * k + j] = s->topk_id_host[i * TOPK_MAX + j];
        top_logprobs[i * k + j] = s->topk_lp_host[i * TOPK_MAX + j];
      }
    s->last_use_mask = use_mask;
    s->last_had_logits = 1;
  }
  tm_step.collect();
  if (tm_step.on) profile().ms[4] += 1;
  WB_HIP(hipGetLastError());
  s->prev_len = len;
  s->prev_win.assign(window, window + n);
  s->prev_n = n;
  s->step++;
  return WB_OK;
}

}  // extern "C"
