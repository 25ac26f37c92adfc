// Device-chained greedy decode: the persistent flag-chained launch (decode_persist.hip) and the graph-replayed chain of one
// launch per sublayer behind it.
#include <climits>
#include <cstring>
#include <string>

#include "decode_step.h"
#include "handoff.h"
#include "switches.h"

using namespace wb;

namespace wb {

// Pinned host words of a greedy call (session.h: ps_pin): the control block's seed, then the words the host reads back.
struct PsPin { size_t seed, err, gctl, tok, total, ctl_ints; };
static PsPin ps_pin_layout(size_t ctl_ints, size_t tok_ints) {
  PsPin p;
  p.seed = 0; p.err = (ctl_ints + 3) & ~(size_t)3; p.gctl = p.err + 4; p.tok = p.gctl + ((ctl_ints + 3) & ~(size_t)3);
  p.total = p.tok + tok_ints; p.ctl_ints = ctl_ints;
  return p;
}
static int ps_pin_ensure(wb_session* s, size_t ints) {
  if (s->ps_pin_ints >= ints) return WB_OK;
  if (s->ps_pin_busy) { WB_HIP(hipStreamSynchronize(s->st)); s->ps_pin_busy = false; }
  if (s->ps_pin) { (void)hipHostFree(s->ps_pin); s->ps_pin = nullptr; s->ps_pin_ints = 0; }
  WB_HIP(hipHostMalloc((void**)&s->ps_pin, ints * 4, hipHostMallocDefault));
  s->ps_pin_ints = ints;
  return WB_OK;
}

// One step's roles, dealt to the blocks: every block runs its own list, in dependency order, every step (decode.h).
//
// A block that holds a first-layer self- or cross-attention role ("early") is the first to be needed in the next step: it
// should be back at its wait, weights and cached K/V requested, before this step ends.  A role of the step's tail on such
// a block delays those requests to the step boundary, and the block's counter poll then queues behind them (vector loads
// return in order).  PS_DEAL_LEGACY dealt finln and merge to "the least loaded blocks", which on a full grid are blocks
// 0 .. W - 1 for the merge roles -- the self-attention roles of row 0's first heads.  PS_DEAL_SLACK: merge(r) goes behind
// finln(r) (that role requests only LayerNorm parameters before its wait, so starting it at the step boundary costs
// nothing), else to a block that is not early and holds no logits role, else to any block that is not early; finln
// prefers blocks that are not early in the same way.  Only where every block is early (small grids) the least loaded ones.
PsDeal ps_deal_roles(int NL, int H, int W, int NB, int n_tiles, int grid, int policy, bool res_on, bool finln) {
  std::vector<PsRole> lr;                            // the layer roles in dependency order
  for (int l = 0; l < NL; l++) {
    for (int r = 0; r < W; r++) for (int h = 0; h < H; h++) lr.push_back(PsRole{PSR_ATTN, l, h, r});
    for (int r = 0; r < W; r++) for (int h = 0; h < H; h++) lr.push_back(PsRole{PSR_CROSS, l, h, r});
    for (int j = 0; j < NB; j++) lr.push_back(PsRole{PSR_MLP, l, j, 0});
  }
  std::vector<std::vector<PsRole>> deal(grid);
  for (size_t i = 0; i < lr.size(); i++) deal[i % grid].push_back(lr[i]);
  // logits: blocks that hold a first-layer attention role stay free of it (see above).  Every logits block takes a run of
  // consecutive 128-column tiles behind ONE fold + LayerNorm.
  std::vector<char> early(grid, 0);
  std::vector<int> cand;
  for (int b = 0; b < grid; b++) {
    for (const PsRole& r : deal[b]) early[b] |= r.layer == 0 && (r.kind == PSR_ATTN || r.kind == PSR_CROSS);
    if (!early[b]) cand.push_back(b);
  }
  if ((int)cand.size() * 4 < n_tiles) { cand.clear(); for (int b = 0; b < grid; b++) cand.push_back(b); }
  const bool slack = policy != PS_DEAL_LEGACY;
  // blocks by load (stable: the lower block first); with `slack`, the ones that are not early before the early ones
  auto by_load = [&](std::vector<int>& v) {
    std::stable_sort(v.begin(), v.end(), [&](int x, int y) {
      if (slack && early[x] != early[y]) return early[x] < early[y];
      return deal[x].size() < deal[y].size();
    });
  };
  // final LayerNorm (one per row): blocks without any layer role if there are some (they sit between the last MLP and
  // the logits on the critical path), else the least loaded ones; they take no logits work
  std::vector<int> fin_block(W, 0);
  std::vector<char> is_fin(grid, 0);
  {
    std::vector<int> order(grid);
    for (int b = 0; b < grid; b++) order[b] = b;
    by_load(order);
    // (without final-LN roles -- the logits roles normalise -- the same blocks stay free of logits tiles for the merge roles)
    for (int r = 0; r < W; r++) {
      fin_block[r] = order[r % grid];
      if (finln) deal[fin_block[r]].push_back(PsRole{PSR_FINLN, 0, 0, r});
      is_fin[fin_block[r]] = 1;
    }
  }
  if ((int)cand.size() > 2 * W) cand.erase(std::remove_if(cand.begin(), cand.end(), [&](int b) { return is_fin[b] != 0; }), cand.end());
  std::stable_sort(cand.begin(), cand.end(), [&](int x, int y) { return deal[x].size() < deal[y].size(); });
  int tpb = (n_tiles + (int)cand.size() - 1) / (int)cand.size();
  // Without final-LN roles the rows are there as soon as the last layer's MLP roles have finished, and a block that holds one of
  // those requests its E^T tiles only then: with two tiles its wait's poll queued ~5 us behind them and it finished the step's
  // logits 6 us after everybody else (profiles/r22_ps_timeline_tree_deal0.txt).  Such a block takes ONE tile where the others
  // can absorb the rest without a longer run (bench shape: 24 x 1 + 191 x 2 = 406 tiles on 215 of the 217 eligible blocks).
  std::vector<char> late(grid, 0);
  int n_late = 0;
  if (!finln && tpb > 1) {
    for (int b : cand) {
      for (const PsRole& r : deal[b]) late[b] |= r.kind == PSR_MLP && r.layer == NL - 1;
      n_late += late[b];
    }
    const int n_other = (int)cand.size() - n_late;
    if (n_late == 0 || n_other <= 0 || (n_tiles - n_late + n_other - 1) / n_other > tpb) { std::fill(late.begin(), late.end(), 0); n_late = 0; }
  }
  std::vector<char> has_lg(grid, 0);
  int n_lg = 0;
  for (int q = 0, t0 = 0; q < (int)cand.size() && t0 < n_tiles; q++) {
    const int n = std::min(late[cand[q]] ? 1 : tpb, n_tiles - t0);
    deal[cand[q]].push_back(PsRole{PSR_LOGITS, n_lg++, t0, n});
    has_lg[cand[q]] = 1;
    t0 += n;
  }
  // merge (one per row)
  {
    std::vector<int> order;
    if (slack) {
      for (int b = 0; b < grid; b++) if (!early[b] && !has_lg[b]) order.push_back(b);
      if (order.empty()) for (int b = 0; b < grid; b++) if (!early[b]) order.push_back(b);
    }
    if (order.empty()) for (int b = 0; b < grid; b++) order.push_back(b);
    by_load(order);
    for (int r = 0; r < W; r++) {
      const int b = slack && !early[fin_block[r]] ? fin_block[r] : order[r % (int)order.size()];
      deal[b].push_back(PsRole{PSR_MERGE, 0, 0, r});
    }
  }
  PsDeal out;
  out.n_lg = n_lg;
  out.tail_block = fin_block;
  out.role_off.assign(grid + 1, 0);
  for (int b = 0; b < grid; b++) {
    out.role_off[b] = (int)out.roles.size();
    out.roles.insert(out.roles.end(), deal[b].begin(), deal[b].end());
  }
  out.role_off[grid] = (int)out.roles.size();
  // Resident operands (WHISPER_HIP_PERSIST_RESIDENT, default on; "0": off; "log": on, and one line on stderr): a block whose
  // list holds exactly ONE layer role, a self- or cross-attention one, runs that role every step -- the kernel keeps what
  // fits of the role's step-invariant operands in the LDS the roles leave free.  Blocks with several layer roles (a grid
  // smaller than the layer roles) would have to share the region: they run as before.
  out.res_role.assign(grid, -1);                    // per block: the index of its resident role
  if (res_on)
    for (int b = 0; b < grid; b++) {
      int n_lr = 0, at = -1;
      for (int i = out.role_off[b]; i < out.role_off[b + 1]; i++)
        if (out.roles[i].kind <= PSR_MLP) { n_lr++; at = i; }
      if (n_lr == 1 && out.roles[at].kind != PSR_MLP) { out.res_role[b] = at; out.n_res++; }
    }
  return out;
}

// Blocks of the persistent launch of this session: what is co-resident, but never more than one step has roles.  The one place
// the grid is computed: the dealing and the choice of the MLP form (two phases need nb_mlp <= grid) both rest on it.
static int ps_grid_blocks(const wb_session* s) {
  const wb_dims& D = s->m->dims;
  const int NB = dec_mlp_fused_planes(D.n_text_state), n_tiles = (D.n_vocab + 127) / 128;
  const int n_layer_roles = D.n_text_layer * (2 * s->W * D.n_text_head + NB);
  return std::max(1, std::min(s->ps_grid, n_layer_roles + n_tiles + 2 * s->W));
}

// WHISPER_HIP_PERSIST_DEAL=log: where the roles of the step's tail went and which MLP form runs, one line per built setup
static void ps_deal_log(const PsDeal& deal, int grid, bool finln) {
  std::string where[2];
  int n_lg_blocks = 0;
  // (two-phase form, no final-LN roles: "finln on" lists the blocks kept free of logits tiles for the rows' merge roles)
  if (!finln) for (int b : deal.tail_block) where[1] += (where[1].empty() ? "" : ",") + std::to_string(b);
  for (int b = 0; b < grid; b++) {
    bool lg = false;
    for (int i = deal.role_off[b]; i < deal.role_off[b + 1]; i++) {
      const int k = deal.roles[i].kind;
      lg |= k == PSR_LOGITS;
      if (k == PSR_MERGE || k == PSR_FINLN) {
        std::string& w = where[k == PSR_FINLN];
        w += (w.empty() ? "" : ",") + std::to_string(b);
      }
    }
    n_lg_blocks += lg;
  }
  fprintf(stderr, "persist deal: merge on blocks %s; finln on %s; logits blocks %d; mlp form %s\n", where[0].c_str(), where[1].c_str(),
          n_lg_blocks, finln ? "planes (final-LN roles)" : "two-phase (no final-LN role: final LayerNorm inside the logits roles)");
}

// The launch setup of the persistent kernel: the per-layer argument blocks -- exactly what enqueue_step hands the fused
// sublayer kernels -- and one step's roles dealt to the blocks, on the device (ps_layers, ps_roles).  All of it is a function
// of the model (and its LayerNorm variant), the session's buffers, W, the grid, the window geometry, the resident switch and the dealing
// policy (what varies from call to call travels by value in PersistArgs), so a pooled session in a transcription loop builds and
// uploads it once: it is kept under a key that names everything it was built from.  WHISPER_HIP_PERSIST_SETUP=0: built and
// uploaded on every call (A/B runs); "log": one line per launch on stderr ("0log": both).  *built: this call built it (and
// waited for the upload: the staging is on the stack).
static int ps_setup_ensure(wb_session* s, bool res_on, bool mlp2, bool* built) {
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int d = D.n_text_state, H = D.n_text_head, NL = D.n_text_layer, V = D.n_vocab, S = s->S, W = s->W;
  const StepLayout& L = s->lay;
  hipStream_t st = s->st;
  const int NB = dec_mlp_fused_planes(d);
  const int n_tiles = (V + 127) / 128;
  const size_t pool = (size_t)s->Lmax * S;
  const int ldkv = 2 * d;
  const int n_pass = s->maxC > CROSS_FUSED_MAX_C ? 2 : 1;
  const int grid = ps_grid_blocks(s);
  const char* deal_sw = sw::persist_deal();
  const int policy = deal_sw && !strcmp(deal_sw, "legacy") ? PS_DEAL_LEGACY : PS_DEAL_SLACK;
  auto up = [](const void* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); };
  const std::vector<uint64_t> key = {
      s->model_uid, (uint64_t)W, (uint64_t)S, (uint64_t)s->Lmax, (uint64_t)grid, (uint64_t)n_tiles, (uint64_t)n_pass,
      (uint64_t)s->enc_rows, (uint64_t)res_on, (uint64_t)m->ln_eps_inside_sqrt, up(s->state.p), up(s->x.p), up(s->P2.p),
      up(s->Pa.p), up(s->Pc.p), up(s->kc.p), up(s->vc.p), up(s->tabs.p), up(s->ckv.p), up(s->win_meta.p), up(s->ps_gx.p),
      up(s->ps_gpa.p), up(s->ps_gpc.p), up(s->ps_gp2.p), up(s->ps_gxn.p), (uint64_t)policy, (uint64_t)mlp2};
  const char* sw_setup = sw::persist_setup();
  const bool cache_on = !(sw_setup && sw_setup[0] == '0');
  *built = !(cache_on && !s->ps_setup_key.empty() && s->ps_setup_key == key);
  if (sw_setup && strstr(sw_setup, "log")) fprintf(stderr, "persist setup: %s\n", *built ? "built" : "reused");
  if (!*built) return WB_OK;
  s->ps_setup_key.clear();                           // void the cache key before the contents change
  char* gxb[2] = {static_cast<char*>(s->ps_gx.p), static_cast<char*>(s->ps_gx.p) + (size_t)S * d * 8};
  std::vector<PsLayerArgs> la(NL);
  float* xb[2] = {s->x.as<float>(), s->x.as<float>() + (size_t)S * d};
  int xi = 0;
  for (int l = 0; l < NL; l++) {
    const DecBlockW& b = m->dec[l];
    AttnFusedArgs& fa = la[l].attn;
    fa.st = s->state.as<int>(); fa.lay = L; fa.S = S; fa.d = d; fa.n_head = H;
    fa.x_in = xb[xi]; fa.pend = l == 0 ? nullptr : s->P2.as<float>(); fa.KSp = l == 0 ? 0 : NB;
    fa.pbias = l == 0 ? nullptr : m->dec[l - 1].mlp2.b; fa.x_out = xb[xi ^ 1];
    fa.ln_g = b.ln1.g; fa.ln_b = b.ln1.b; fa.ln_eps = b.ln1.eps; fa.ln_inside = m->ln_eps_inside_sqrt;
    fa.Wqkv = b.qkv.w; fa.ldqkv = b.qkv.n; fa.bqkv = b.qkv.b; fa.scale = m->qk_scale;
    fa.Kc = s->kc.as<float>() + (size_t)l * pool * d; fa.Vc = s->vc.as<float>() + (size_t)l * pool * d;
    fa.tabs = s->tabs.as<int>(); fa.Lmax = s->Lmax; fa.Wo = b.out.w; fa.P = s->Pa.as<float>();
    fa.g_x_in = gxb[xi]; fa.g_pend = l == 0 ? nullptr : s->ps_gp2.p; fa.g_x_out = gxb[xi ^ 1]; fa.g_P = s->ps_gpa.p;
    xi ^= 1;
    CrossFusedArgs& ca = la[l].cross;
    ca.st = s->state.as<int>(); ca.lay = L; ca.S = S; ca.d = d; ca.n_head = H;
    ca.x_in = xb[xi]; ca.pend = s->Pa.as<float>(); ca.KSp = H; ca.pbias = b.out.b; ca.x_out = xb[xi ^ 1];
    ca.ln_g = b.ln2.g; ca.ln_b = b.ln2.b; ca.ln_eps = b.ln2.eps; ca.ln_inside = m->ln_eps_inside_sqrt;
    ca.Wq = b.cq.w; ca.bq = b.cq.b; ca.scale = m->qk_scale;
    ca.ckv = s->ckv.as<float>() + (size_t)l * s->enc_rows * 2 * d; ca.ldkv = ldkv; ca.koff = 0;   // layer-major cached K|V
    ca.win_row0 = s->win_meta.as<int>(); ca.win_C = s->win_meta.as<int>() + W;
    ca.Wo = b.cout.w; ca.P = s->Pc.as<float>();
    ca.n_pass = n_pass;
    ca.g_x_in = gxb[xi]; ca.g_pend = s->ps_gpa.p; ca.g_x_out = gxb[xi ^ 1]; ca.g_P = s->ps_gpc.p;
    xi ^= 1;
    MlpFusedArgs& ma = la[l].mlp;
    ma.st = s->state.as<int>(); ma.S = S; ma.d = d;
    ma.x_in = xb[xi]; ma.pend = s->Pc.as<float>(); ma.KSp = H; ma.pbias = b.cout.b; ma.x_out = xb[xi ^ 1];
    ma.ln_g = b.ln3.g; ma.ln_b = b.ln3.b; ma.ln_eps = b.ln3.eps; ma.ln_inside = m->ln_eps_inside_sqrt;
    ma.W1 = b.mlp1.w; ma.ld1 = b.mlp1.n; ma.b1 = b.mlp1.b; ma.W2 = b.mlp2.w; ma.P = s->P2.as<float>();
    ma.g_x_in = gxb[xi]; ma.g_pend = s->ps_gpc.p; ma.g_x_out = gxb[xi ^ 1]; ma.g_P = s->ps_gp2.p;
    la[l].mlp_b2 = b.mlp2.b;
    xi ^= 1;
  }
  // ---- one step's roles, dealt to the blocks: every block runs its own list, in dependency order, every step ----
  PsDeal deal = ps_deal_roles(NL, H, W, NB, n_tiles, grid, policy, res_on, !mlp2);
  if (deal_sw && !strcmp(deal_sw, "log")) ps_deal_log(deal, grid, !mlp2);
  std::vector<PsRole>& roles = deal.roles;
  const std::vector<int>&role_off = deal.role_off, &res_role = deal.res_role;
  const int n_lg = deal.n_lg, n_res = deal.n_res;
  WB_TRY(s->ps_layers.ensure(la.size() * sizeof(PsLayerArgs)));
  WB_TRY(s->ps_roles.ensure(roles.size() * sizeof(PsRole) + (role_off.size() + res_role.size()) * 4));
  WB_HIP(hipMemcpyAsync(s->ps_layers.p, la.data(), la.size() * sizeof(PsLayerArgs), hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(s->ps_roles.p, roles.data(), roles.size() * sizeof(PsRole), hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(static_cast<char*>(s->ps_roles.p) + roles.size() * sizeof(PsRole), role_off.data(), role_off.size() * 4,
                        hipMemcpyHostToDevice, st));
  WB_HIP(hipMemcpyAsync(static_cast<char*>(s->ps_roles.p) + roles.size() * sizeof(PsRole) + role_off.size() * 4, res_role.data(),
                        res_role.size() * 4, hipMemcpyHostToDevice, st));
  WB_HIP(hipStreamSynchronize(st));            // (the staging vectors above are on the stack)
  s->ps_pin_busy = false;
  s->ps_roles_host.swap(roles);
  s->ps_role_off_host = role_off;
  s->ps_setup_grid = grid; s->ps_setup_n_lg = n_lg; s->ps_setup_n_res = n_res;
  s->ps_setup_key = key;
  return WB_OK;
}

// The whole chained greedy decode as ONE persistent launch (decode_persist.hip): every sublayer of every step runs in a
// co-resident grid whose blocks hand their output planes to each other through arrival counters.  Enqueues the zeroing of the
// polled words, the first step's prepare kernel and the launch behind whatever the stream still holds (the encoder: with the
// launch setup cached nothing here waits for it), copies the words the host needs into pinned memory (ps_pin: error word,
// control block, token rows) and waits for the stream ONCE.  *steps_done = steps executed.
//
// *fell_back: the launch was refused (no cooperative launch on this device / partition, the grid not co-resident, a
// second cooperative client) or a wait gave up before ANY step was committed -- the caller re-seeds the control block and
// runs the graph-replayed chain of one launch per sublayer instead (it derives everything from gctl), and the session
// stops trying the persistent kernel.  A wait that gives up after steps were committed stays an error.
static int run_persistent_chain(wb_session* s, int eot, int max_depth, int mask_until_len, const int32_t* forced, int n_forced,
                                const PsPin& pin, int* steps_done, bool* fell_back) {
  *fell_back = false;
  WB_REQUIRE(n_forced >= 0 && n_forced <= PS_MAX_FORCED, WB_ERR_ARG, "persistent decode: %d prompt steps", n_forced);
  // test hook (tests/test_emu_functional.py, tests/test_gpu_switches.py): "launch" = behave as if the cooperative launch was refused
  const char* inject = sw::persist_inject_fail();
  wb_model* m = s->m;
  const wb_dims& D = m->dims;
  const int d = D.n_text_state, H = D.n_text_head, NL = D.n_text_layer, V = D.n_vocab, S = s->S, W = s->W;
  const StepLayout& L = s->lay;
  hipStream_t st = s->st;
  const int NB = dec_mlp_fused_planes(d);
  const int n_tiles = (V + 127) / 128;
  // ---- the hand-off buffers: residual streams and partial planes as {tag, value} granules (zero-filled once: tag 0 is
  // never used; the tags of a launch live above launch_count << 16, so leftovers of earlier decodes never match)
  WB_REQUIRE(NB <= 32 && H <= 8, WB_ERR_SHAPE, "persistent decode: more planes than its folds hold");
  WB_TRY(s->ps_gx.ensure_zeroed(((size_t)2 * S + 8) * d * 8, st));
  WB_TRY(s->ps_gpa.ensure_zeroed(((size_t)H * S + 8) * d * 8, st));
  WB_TRY(s->ps_gpc.ensure_zeroed(((size_t)H * S + 8) * d * 8, st));
  // WHISPER_HIP_PERSIST_MLP=planes: the MLP roles leave 4 d / 64 partial planes per layer and a final-LN role folds the last
  // layer's (the A/B arm); unset: two-phase MLP roles, final LayerNorm inside the logits roles.  The dealt roles depend on it.
  // Phase 2 of an MLP role waits for the hidden values of ALL 4 d / 64 MLP roles of its layer, so those must sit on different
  // blocks (layer role i is dealt to block i % grid: they do when the grid has at least that many blocks).  On a smaller grid a
  // block would wait for a role further down its own list: the planes form, whose roles depend on earlier stages only
  // (WHISPER_HIP_PERSIST_DEAL=log names the form that runs).
  const char* mlp_sw = sw::persist_mlp();
  const bool mlp2 = !(mlp_sw && !strcmp(mlp_sw, "planes")) && ps_grid_blocks(s) >= NB;
  if (mlp2) {
    WB_TRY(s->ps_ghid.ensure_zeroed(((size_t)S + 2) * 4 * d * 8, st));
  } else {                                         // (the planes and the final-LN rows exist in the planes form only)
    WB_TRY(s->ps_gp2.ensure_zeroed(((size_t)NB * S + 8) * d * 8, st));
    WB_TRY(s->ps_gxn.ensure_zeroed(((size_t)S + 8) * d * 8, st));
  }
  WB_TRY(s->ps_tstats.ensure_zeroed((size_t)2 * S * n_tiles * 16, st));   // tile records, tagged like granules, two step parities
  if (((s->ps_launches + 1) & 0xffffu) == 0) {     // the 16-bit launch count wraps: forget every old tag
    for (DevMem* b : {&s->ps_gx, &s->ps_gpa, &s->ps_gpc, &s->ps_gp2, &s->ps_gxn, &s->ps_ghid, &s->ps_tstats})
      if (b->p && b->bytes) WB_HIP(hipMemsetAsync(b->p, 0, b->bytes, st));
    s->ps_launches++;
  }
  const unsigned tag_base = ((++s->ps_launches) & 0xffffu) << 16;
  char* gxb[2] = {static_cast<char*>(s->ps_gx.p), static_cast<char*>(s->ps_gx.p) + (size_t)S * d * 8};
  // ---- per-layer arguments and the dealt roles: on the device, built only when what they were built from has changed ----
  const char* res_sw = sw::persist_resident();
  const bool res_on = !(res_sw && res_sw[0] == '0') && dec_persist_resident_slots(d, W, s->maxC) > 0;
  bool built = false;
  WB_TRY(ps_setup_ensure(s, res_on, mlp2, &built));
  const std::vector<PsRole>& roles = s->ps_roles_host;
  const int grid = s->ps_setup_grid, n_res = s->ps_setup_n_res;
  if (res_sw && !strcmp(res_sw, "log")) fprintf(stderr, "persist resident blocks: %d of %d\n", n_res, grid);
  const int n_ctl = ps_ctl_ints(S, NL);
  WB_TRY(s->ps_ctl.ensure((size_t)n_ctl * 4));
  WB_TRY(s->ps_dead.ensure((size_t)S * 4));
  // the polled words start at zero; HX_STOP = INT_MAX is written by the seed kernel below
  WB_HIP(hipMemsetAsync(s->ps_ctl.p, 0, (size_t)n_ctl * 4, st));
  WB_HIP(hipMemsetAsync(s->ps_dead.p, 0, (size_t)S * 4, st));
  PersistArgs a;
  a.layers = s->ps_layers.as<PsLayerArgs>(); a.roles = s->ps_roles.as<PsRole>(); a.n_roles = (int)roles.size();
  a.role_off = reinterpret_cast<const int*>(static_cast<char*>(s->ps_roles.p) + roles.size() * sizeof(PsRole));
  if (n_res > 0) a.res_role = a.role_off + (grid + 1);
  a.n_logits_roles = s->ps_setup_n_lg;
  a.n_layer = NL; a.n_rows = W; a.S = S; a.d = d; a.n_head = H; a.nb_mlp = NB;
  a.n_pass = s->maxC > CROSS_FUSED_MAX_C ? 2 : 1;
  a.ctl = s->ps_ctl.as<int>(); a.step0 = s->step; a.n_steps = n_forced + max_depth; a.mask_until_len = mask_until_len;
  a.n_forced = n_forced;
  for (int i = 0; i < n_forced; i++) a.forced[i] = forced[i];
  a.g_xn = s->ps_gxn.p;
  a.mlp2 = mlp2 ? 1 : 0; a.g_hid = s->ps_ghid.p;
  a.x_fin = gxb[(3 * NL) & 1]; a.P2 = s->ps_gp2.p; a.b2_last = m->dec[NL - 1].mlp2.b; a.tag_base = tag_base;
  a.ln_g = m->ln_dec.g; a.ln_b = m->ln_dec.b; a.ln_eps = m->ln_dec.eps; a.ln_inside = m->ln_eps_inside_sqrt;
  a.Et = m->tok_emb_t; a.vocab_ld = m->vocab_ld; a.V = V; a.mask = s->mask.as<float>();
  a.tstats = s->ps_tstats.p; a.n_tiles = n_tiles;
  // WHISPER_HIP_PERSIST_PICK=merge: first-layer self-attention waits for the merge role's x row (the A/B arm); unset: it picks
  // the token from the tile records itself.  A word of the launch's arguments: the dealt tables do not depend on it
  const char* pick_sw = sw::persist_pick();
  a.pick = pick_sw && !strcmp(pick_sw, "merge") ? 0 : 1;
  a.gctl = s->gctl.as<int>(); a.gtok = s->gtok.as<int>(); a.Lmax = s->Lmax; a.eot = eot;
  a.E = m->tok_emb; a.pos = m->dec_pos; a.x0 = gxb[0]; a.tabs = s->tabs.as<int>(); a.dead = s->ps_dead.as<int>();
  // optional role timeline (developer): WHISPER_HIP_PS_STAMPS=<file> dumps [n_steps][n_roles][3] 100 MHz clock values
  const char* stamps_path = sw::ps_stamps();
  const size_t n_stamps = stamps_path ? (size_t)(n_forced + max_depth) * roles.size() * 8 : 0;
  if (n_stamps) {
    WB_TRY(s->ps_stamps.ensure(n_stamps * 8));
    WB_HIP(hipMemsetAsync(s->ps_stamps.p, 0, n_stamps * 8, st));
    a.stamps = s->ps_stamps.as<unsigned long long>();
  }
  WB_REQUIRE(3 * NL * (n_forced + max_depth + 1) + 4 < 0x10000, WB_ERR_SHAPE,
             "persistent decode: %d layers x %d steps do not fit the 16-bit granule tags", NL, max_depth);
  // first step of the chain: token + position embedding of the last prompt token (every later step: the merge role)
  launch_dec_prepare(st, reinterpret_cast<const int*>(s->host_block_dev), s->state.as<int>(), L, W, s->tabs.as<int>(),
                     s->Lmax, m->tok_emb, m->dec_pos, d, s->x.as<float>(), s->gctl.as<int>());
  launch_ps_seed(st, s->x.as<float>(), W * d, gxb[0], tag_base + 1u, s->ps_ctl.as<int>());
  hipEvent_t e0 = nullptr, e1 = nullptr;
  prof_tag(KC_PERSIST, 0.0);                   // (its necessary bytes are known when the rows' lengths are: added by the caller)
  const bool timed = prof_take_events(&e0, &e1);
  if (timed) WB_HIP(hipEventRecord(e0, st));
  const bool refused = (inject && !strcmp(inject, "launch")) || launch_dec_persist(st, a, grid) != 0;
  if (timed) WB_HIP(hipEventRecord(e1, st));
  if (refused) {
    (void)hipGetLastError();                   // (clears the sticky launch error)
    s->ps_grid = 0;
    *fell_back = true;
    *steps_done = 0;
    return WB_OK;
  }
  // what the host needs, into pinned memory, behind one synchronisation: the error word, the control block (GC_STEP: steps
  // committed) and the token rows
  int* hp = s->ps_pin;
  s->ps_pin_busy = true;
  WB_HIP(hipMemcpyAsync(hp + pin.err, s->ps_ctl.as<int>() + HX_ERR, 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(hp + pin.gctl, s->gctl.p, pin.ctl_ints * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipMemcpyAsync(hp + pin.tok, s->gtok.p, (pin.total - pin.tok) * 4, hipMemcpyDeviceToHost, st));
  WB_HIP(hipStreamSynchronize(st));
  s->ps_pin_busy = false;
  const int err = hp[pin.err], gstep = hp[pin.gctl + GC_STEP];
  if (err != 0 && gstep == s->step) {          // nothing committed: the chain can take over from the same control block
    s->ps_grid = 0;
    *fell_back = true;
    *steps_done = 0;
    return WB_OK;
  }
  WB_REQUIRE(err == 0, WB_ERR_HIP, "persistent decode: a wait gave up (counter %d) at step %d", err - 1, gstep);
  if (n_stamps) {
    std::vector<unsigned long long> hs(n_stamps);
    WB_HIP(hipMemcpy(hs.data(), s->ps_stamps.p, n_stamps * 8, hipMemcpyDeviceToHost));
    if (FILE* f = fopen(stamps_path, "wb")) {
      const int hdr[4] = {n_forced + max_depth, (int)roles.size(), grid, 8};
      fwrite(hdr, 4, 4, f);
      std::vector<int> kinds(roles.size());
      for (size_t i = 0; i < roles.size(); i++)
        kinds[i] = roles[i].kind | ((roles[i].kind <= PSR_MLP ? roles[i].layer : 0) << 8) |
                   ((roles[i].kind == PSR_LOGITS ? 0 : roles[i].b) << 16);
      fwrite(kinds.data(), 4, kinds.size(), f);
      fwrite(hs.data(), 8, hs.size(), f);
      // behind what older readers expect: a marker, then role_off (which block ran which role)
      const int marker = 0x66664f52;                 // "ROff"
      fwrite(&marker, 4, 1, f);
      fwrite(s->ps_role_off_host.data(), 4, s->ps_role_off_host.size(), f);
      fclose(f);
    }
  }
  *steps_done = std::max(0, std::min(n_forced + max_depth, gstep - s->step));
  return WB_OK;
}

// Device-chained greedy decode (beam_size == 1): after the host-driven prompt prefill, every step's
// argmax is fed to the next step on the device; the host only replays the step graph and checks the
// per-window finished flags every `chunk` steps.  Equivalent to beam.rs with k = 1: the single beam is
// extended by its best continuation (lowest id on ties) until it ends in EOT or max_depth tokens.
// A fresh session (step 0) hands in the whole prompt: the persistent kernel runs the prompt's first prompt_len - 1 positions as
// forced steps of the same launch (no host round trip between the prompt and the first generated token); the chain of one
// launch per sublayer (and the persistent kernel's fallback) prefills through host-driven steps first, as before.
int session_greedy_chain(wb_session* s, const int32_t* prompt, int eot, int max_depth, int mask_until_len, int prompt_len,
                         int32_t* out_tokens, int32_t row_stride, int32_t* out_lens) {
  wb_model* m = s->m;
  const int S = s->S, W = s->W;
  WB_REQUIRE(S == W, WB_ERR_STATE, "chained greedy decode needs max_beams == 1");
  WB_REQUIRE(prompt && prompt_len >= 1, WB_ERR_ARG, "chained greedy decode: empty prompt");
  WB_REQUIRE(s->step == 0 || (s->prev_n == W && s->step == prompt_len - 1), WB_ERR_STATE,
             "chained greedy decode: the session is neither fresh nor prefilled");
  const int n_forced_max = prompt_len - 1;          // prompt positions that can run inside the persistent launch
  auto host_prefill = [&]() -> int {                 // transcribe.rs:203: the prompt, one KV-cached step per token, no logits
    std::vector<int32_t> tok(W), par(W), win(W);
    for (int t = s->step; t < prompt_len - 1; t++) {
      for (int w = 0; w < W; w++) { tok[w] = prompt[t]; par[w] = t == 0 ? -1 : w; win[w] = w; }
      WB_TRY(wb_session_step(s, tok.data(), par.data(), win.data(), W, 0, 0, nullptr, nullptr));
    }
    return WB_OK;
  };
  // the first steps read the special-token mask (transcribe.rs:271-275): same contract as wb_session_step
  WB_REQUIRE(s->has_mask || mask_until_len < prompt_len || max_depth == 0, WB_ERR_STATE,
             "wb_session_decode: special mask not set");
  // The reference only fails (mod.rs:134-139) when a sequence actually outgrows n_text_ctx: a large max_depth
  // whose windows all end on EOT earlier succeeds.  Run at most the steps the context holds; raise the
  // reference's error afterwards if a window is still unfinished.
  const int asked_depth = max_depth;
  max_depth = std::min(max_depth, s->Lmax - (prompt_len - 1));
  WB_HIP(hipSetDevice(m->device));
  hipStream_t st = s->st;
  const size_t ctl_ints = GC_HDR + 3 * (size_t)S;
  WB_TRY(s->gctl.ensure(ctl_ints * 4));
  // token rows [S][Lmax]; the last generated token of a row that fills the context lands at index Lmax
  // (= slot 0 of the next row, a prompt position nobody reads), so the buffer carries one extra slot
  WB_TRY(s->gtok.ensure(((size_t)S * s->Lmax + 1) * 4));
  std::vector<int> ctl(ctl_ints, 0);
  // the seed travels through the session's pinned words: the copy needs no wait for its source, so the persistent launch is
  // enqueued behind the encoder instead of draining it (wait: the chain of one launch per sublayer synchronises as before)
  const PsPin pin = ps_pin_layout(ctl_ints, (size_t)S * s->Lmax + 1);
  WB_TRY(ps_pin_ensure(s, pin.total));
  auto seed_ctl = [&](bool wait) -> int {            // the chain starts at the session's step with that position's prompt token
    if (s->ps_pin_busy) { WB_HIP(hipStreamSynchronize(st)); s->ps_pin_busy = false; }
    int* seed = s->ps_pin + pin.seed;
    std::fill(seed, seed + ctl_ints, 0);
    seed[GC_STEP] = s->step;
    for (int i = 0; i < W; i++) seed[GC_HDR + i] = prompt[s->step];
    s->ps_pin_busy = true;
    WB_HIP(hipMemcpyAsync(s->gctl.p, seed, ctl_ints * 4, hipMemcpyHostToDevice, st));
    if (wait) { WB_HIP(hipStreamSynchronize(st)); s->ps_pin_busy = false; }
    return WB_OK;
  };
  const StepPlan plan = plan_step(s, W, false);     // (no 9 - 16-row fused bucket here: W in 9..16 is batch mode)
  const int n_launch = plan.n_launch;
  const bool fuse_ln = plan.fuse_ln;
  const int chunk = 16;
  int depth = 0;                                   // steps enqueued so far
  bool persist = plan.persist && max_depth > 0;
  if (persist) {
    if (s->ps_grid < 0) s->ps_grid = dec_persist_max_grid(m->device, m->dims.n_text_state, W, s->maxC);
    persist = s->ps_grid > 0;
  }
  // prompt positions the persistent launch runs itself (a fresh session; WHISPER_HIP_PERSIST_PREFILL=0: host-driven prefill)
  int n_forced = 0;
  if (s->step == 0 && s->prefill_mode == 1 && sw::prefill_pass() && prompt_len > 1) {
    // one-pass prompt prefill (prefill.cpp): the session is "prefilled" afterwards, so the launch below forces nothing
    std::vector<int> win(W);
    for (int w = 0; w < W; w++) win[w] = w;
    WB_TRY(session_prefill(s, prompt, prompt_len - 1, win.data(), W));
  }
  if (persist && sw::persist_prefill() && s->step == 0 && n_forced_max <= PS_MAX_FORCED && s->has_mask) n_forced = n_forced_max;
  if (n_forced == 0) WB_TRY(host_prefill());
  WB_TRY(seed_ctl(!persist));
  ScopedTimer tm(st, 3);
  if (persist) {
    bool fell_back = false;
    WB_TRY(run_persistent_chain(s, eot, max_depth, mask_until_len, prompt + s->step + 1, n_forced, pin, &depth, &fell_back));
    if (fell_back) {
      // rows whose merge role ran before the give-up have moved their control words: prefill on the host (if the launch was
      // to do it) and start the chain over from the seed
      persist = false;
      depth = 0;
      WB_TRY(host_prefill());
      WB_TRY(seed_ctl(true));
      n_forced = 0;
    } else {
      if (profile().on) profile().ms[4] += depth;
      depth -= n_forced;                             // from here on `depth` counts GENERATED positions
      s->step += n_forced;
      s->prev_n = W;
      s->prev_win.resize(W);
      for (int w = 0; w < W; w++) s->prev_win[w] = w;
    }
  }
  if (!persist) {
  if (fuse_ln)   // first step of the chain; every later one is prepared by its predecessor's merge kernel
    launch_dec_prepare(st, reinterpret_cast<const int*>(s->host_block_dev), s->state.as<int>(), s->lay, n_launch,
                       s->tabs.as<int>(), s->Lmax, m->tok_emb, m->dec_pos, m->dims.n_text_state, s->x.as<float>(),
                       s->gctl.as<int>());
  // masked steps (the first two, transcribe.rs:271-275) and the tail shorter than a chunk go one step per
  // graph launch; in between, a whole chunk of steps is ONE graph launch (two multi-step shapes are never
  // needed: only {1 step masked, 1 step, chunk steps} are captured).
  //
  // Small batches (the fused-LayerNorm path) run one segment AHEAD of the finished flags: segment k + 1 is enqueued
  // before the flags of segment k are read (on a second stream, behind an event), so the GPU never idles across
  // the host round trip (~60-400 us per check in round 1's timeline).  If every window turns out to be finished,
  // the merge kernel has already blanked the step state (ST_N = 0) and the kernels of the speculative segment exit
  // at their first instruction.  Batch mode (> 8 rows: MFMA GEMMs that do not look at ST_N) keeps the blocking check.
  // (opt-in: measured 1417x vs 1543x -- a graph launched behind a running graph starts later than one launched on an
  // idle stream saves)
  const bool speculate = fuse_ln && sw::speculate();
  if (speculate && !s->st2) {
    WB_HIP(hipStreamCreateWithFlags(&s->st2, hipStreamNonBlocking));
    WB_HIP(hipEventCreateWithFlags(&s->ev_seg, hipEventDisableTiming));
  }
  auto enqueue_segment = [&](int* enq) -> int {   // >= `chunk` steps (or what is left); returns steps enqueued via *enq
    int n = 0;
    while (depth + n < max_depth && n < chunk) {
      const int d0 = depth + n;
      const int use_mask = (prompt_len + d0) <= mask_until_len ? 1 : 0;
      const int run = (!use_mask && max_depth - d0 >= chunk) ? chunk : 1;
      StepCall call;
      call.k = 1; call.use_mask = use_mask; call.chained = true; call.eot = eot; call.reps = run;
      WB_TRY(launch_step(s, plan, call));
      if (profile().on) profile().ms[4] += run;
      n += run;
    }
    *enq = n;
    return WB_OK;
  };
  auto read_flags = [&](bool behind_event) -> int {
    if (behind_event) {
      WB_HIP(hipStreamWaitEvent(s->st2, s->ev_seg, 0));
      WB_HIP(hipMemcpyAsync(ctl.data(), s->gctl.p, ctl_ints * 4, hipMemcpyDeviceToHost, s->st2));
      WB_HIP(hipStreamSynchronize(s->st2));
    } else {
      WB_HIP(hipMemcpyAsync(ctl.data(), s->gctl.p, ctl_ints * 4, hipMemcpyDeviceToHost, st));
      WB_HIP(hipStreamSynchronize(st));
    }
    return WB_OK;
  };
  auto all_done = [&]() {
    bool d = true;
    for (int i = 0; i < W; i++) d = d && ctl[GC_HDR + S + i] != 0;
    return d;
  };
  // small batches: the merge kernel publishes (steps completed, finished) per row into mapped host memory; the host
  // spins on it (a few us) instead of a D2H copy + stream synchronisation (30-190 us of idle GPU per check in round 1)
  const bool poll = fuse_ln && sw::poll() && !profile().on;
  volatile int* hfl = reinterpret_cast<volatile int*>(s->host_block + s->chain_flags_off);
  if (poll) for (int i = 0; i < 2 * S; i++) hfl[i] = 0;
  auto wait_flags = [&](int want_step, bool* done) -> int {
    for (long spins = 0;; spins++) {
      bool ready = true;
      for (int i = 0; i < W && ready; i++) ready = hfl[2 * i] >= want_step;
      if (ready) break;
      bool fin = true;
      for (int i = 0; i < W && fin; i++) fin = hfl[2 * i + 1] != 0;
      if (fin) break;                              // every window finished: the rest of the chunk is blanked
      if ((spins & 0xfff) == 0xfff) {             // every 4096 spins: is the stream still alive / busy?
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) {                     // stream drained: the flags are final (or the chain ended early)
          bool r2 = true;
          for (int i = 0; i < W && r2; i++) r2 = hfl[2 * i] >= want_step;
          if (r2) break;
          bool all = true;
          for (int i = 0; i < W; i++) all = all && hfl[2 * i + 1] != 0;
          if (all) break;                          // every window finished: later steps were blanked
          set_error("chained decode: the device stopped at step %d of %d", (int)hfl[0], want_step);
          return WB_ERR_HIP;
        }
        if (q != hipErrorNotReady) { set_error("chained decode: %s", hipGetErrorString(q)); return WB_ERR_HIP; }
      }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    bool all = true;
    for (int i = 0; i < W; i++) all = all && hfl[2 * i + 1] != 0;
    *done = all;
    return WB_OK;
  };
  if (!speculate) {
    while (depth < max_depth) {
      int n = 0;
      WB_TRY(enqueue_segment(&n));
      depth += n;
      if (poll) {
        bool done = false;
        WB_TRY(wait_flags(s->step + depth, &done));
        if (done) break;
      } else {
        WB_TRY(read_flags(false));
        if (all_done()) break;
      }
    }
  } else {
    int n_cur = 0;
    WB_TRY(enqueue_segment(&n_cur));
    depth += n_cur;
    while (true) {
      WB_HIP(hipEventRecord(s->ev_seg, st));        // end of the segment whose flags are read next
      int n_next = 0;
      if (depth < max_depth) { WB_TRY(enqueue_segment(&n_next)); depth += n_next; }
      WB_TRY(read_flags(true));
      if (all_done() || n_next == 0) break;
    }
    WB_HIP(hipStreamSynchronize(st));
  }
  }   // (!persist)
  tm.stop();
  std::vector<int> toks_chain;
  const int* toks = s->ps_pin + pin.tok;             // (the persistent launch left control block and token rows in ps_pin)
  if (persist) {
    std::copy(s->ps_pin + pin.gctl, s->ps_pin + pin.gctl + ctl_ints, ctl.begin());
  } else {
    toks_chain.resize((size_t)S * s->Lmax + 1);
    WB_HIP(hipMemcpyAsync(ctl.data(), s->gctl.p, ctl_ints * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipMemcpyAsync(toks_chain.data(), s->gtok.p, toks_chain.size() * 4, hipMemcpyDeviceToHost, st));
    WB_HIP(hipStreamSynchronize(st));
    s->ps_pin_busy = false;
    toks = toks_chain.data();
  }
  tm.collect();
  WB_TRY(dec_split_check(s));
  WB_REQUIRE(ctl[GC_BAD] == 0, WB_ERR_STATE, "a decode step produced a row without a finite log-prob (NaN logits: non-finite "
             "weights or activations); its window was ended on <|endoftext|> on the device and the rows of this call are invalid");
  for (int w = 0; w < W; w++) {
    int len = ctl[GC_HDR + 2 * S + w];                 // prompt + generated (through EOT if it came)
    if (len < prompt_len) len = prompt_len;
    len = std::min(len, prompt_len + max_depth);
    WB_REQUIRE(len <= row_stride, WB_ERR_ARG, "row_stride too small");
    for (int p = prompt_len; p < len; p++) out_tokens[(size_t)w * row_stride + p] = toks[(size_t)w * s->Lmax + p];
    out_lens[w] = len;
  }
  if (profile().on && !persist && s->prof_cls_cross >= 0 && s->prof_cls_self >= 0) {
    // The tags counted every launched row's cached K/V.  A row whose window had already ended is marked dead in the
    // step state: its attention blocks exit at their first wait and stream nothing -- take those bytes back, so that
    // the reported algorithmic bytes are the NECESSARY ones.
    const int dm = m->dims.n_text_state, NL = m->dims.n_text_layer;
    double dead_ckv = 0, dead_self = 0;
    for (int w = 0; w < W; w++) {
      const int live = std::max(0, std::min(out_lens[w] - prompt_len, depth));   // steps in which row w was live
      for (int t = live; t < depth; t++) { dead_ckv += 8.0 * s->C[w] * dm; dead_self += 8.0 * (s->step + t + 1) * dm; }
    }
    prof_adjust_bytes(s->prof_cls_cross, -(double)NL * dead_ckv);
    prof_adjust_bytes(s->prof_cls_self, -(double)NL * dead_self);
  }
  if (profile().on && persist) {
    // necessary bytes of the persistent launch: weights + E^T once per executed step, a row's cached cross K/V and
    // self-attention rows only while its window is live
    const double dm = m->dims.n_text_state, NL = m->dims.n_text_layer;
    double bytes = (double)(depth + n_forced) * 4.0 * NL * 14.0 * dm * dm + (double)depth * 4.0 * (double)m->dims.n_vocab * dm;
    for (int w = 0; w < W; w++)                      // (the prompt positions the launch ran itself: every row is live there)
      for (int t = 0; t < n_forced; t++) bytes += NL * (8.0 * s->C[w] * dm + 8.0 * (t + 1) * dm);
    for (int w = 0; w < W; w++) {
      const int live = std::max(0, std::min(out_lens[w] - prompt_len, depth));
      for (int t = 0; t < live; t++) bytes += NL * (8.0 * s->C[w] * dm + 8.0 * (s->step + t + 1) * dm);
    }
    prof_adjust_bytes(KC_PERSIST, bytes);
  }
  s->prof_step_off = 0;
  s->step += depth;
  s->prev_len.assign(W, s->step);
  s->last_had_logits = 0;
  if (max_depth < asked_depth)
    for (int w = 0; w < W; w++)
      WB_REQUIRE(ctl[GC_HDR + S + w] != 0, WB_ERR_SHAPE, "Token sequence length %d must not exceed %d.", s->Lmax + 1,
                 s->Lmax);
  return WB_OK;
}
}  // namespace wb
