// One decode step of a session: which kernels it runs (StepPlan) and how it is launched (decode_step.cpp).
#pragma once
#include "session.h"

namespace wb {

// Everything that selects a step's kernels, derived in ONE place (plan_step) from the session's shapes, the number of live
// rows and the runtime switches.  The enqueue functions read the plan and derive nothing themselves, so a caller's launch
// shape and the kernels that run in it cannot disagree.
struct StepPlan {
  int n_launch = 0;            // rows the kernels are launched for: bucketed, so that one captured graph serves every step
  int max_nb = 1;              // beams-per-window bucket of the chunked cross-attention kernel
  bool use_graph = false;      // replay captured graphs (off while profiling: tagged launches are eager)
  bool fuse_ln = false;        // small batch: LayerNorm in the consumers' prologue; false = batch mode (its own launch + GEMMs)
  bool g16 = false;            // the 9 - 16-row bucket of the fused sublayer kernels
  // small batch
  bool fuse_sub = false;       // self-attention block and MLP block are one launch each (decode_fused.hip)
  bool fuse_x = false;         // ... and so is the cross-attention sublayer
  bool fuse_q = false;         // chunked cross-attention blocks project their own queries
  bool fuse_co = false;        // ... and apply their head's rows of the out-projection (opt-in)
  bool persist = false;        // the persistent flag-chained kernel serves this shape (dec_persist_max_grid decides the rest)
  // batch mode
  bool skinny = false;         // skinny weight-stream GEMM (decode_batch.hip) instead of the tiled one
  bool cross_stream = false;   // one beam per window: streaming cross-attention, no chunk partials / combine
  bool stream_fused = false;   // ... whose blocks fold, normalise and project their own query
  // split-K planes a producer leaves pending for its consumer
  int ks_mlp = 0;              // small batch: the MLP sublayer's
  int kq = 0, ko = 0, k1 = 0, k2 = 0;   // batch mode: QKV, the d x d projections, lin1, lin2
};
// live_rows: rows the step (or the most a search) can have live.  allow_16row_bucket: false for the chained greedy decode,
// which has no 9 - 16-row fused bucket -- W in 9..16 is batch mode there.
StepPlan plan_step(const wb_session* s, int live_rows, bool allow_16row_bucket);

// device-chained beam search: where a step reads its state block and leaves its top-k rows, and the bookkeeping launch behind it
struct BeamStepIO { const int* state_src; int32_t* topk_id; float* topk_lp; BeamChainArgs upd; };
// device-chained sampling: where a step leaves its (unused) top-1 rows, and the draw + bookkeeping launch behind it
struct SampleStepIO { int32_t* topk_id; float* topk_lp; SampleChainArgs upd; };
// device-chained timestamp decoding: the same, with the timestamp-rules pick + bookkeeping launch (tsrules.hip) behind it
struct TsStepIO { int32_t* topk_id; float* topk_lp; TsChainArgs upd; };
// device-chained beam search under the timestamp rules (tsbeam_chain.cpp): where a step leaves its (unused) top-1 rows, the
// per-row candidates launch and the per-window bookkeeping launch (tsbeam.hip) behind it
struct TsBeamStepIO { int32_t* topk_id; float* topk_lp; TsBeamRowsArgs rows; TsBeamUpdateArgs upd; };

// What varies between launches of one plan.  chained: device-chained greedy steps (position and tokens come from the control
// block); reps > 1: that many consecutive chained steps in one graph; bio: a device-chained beam step; sio: a device-chained
// sampling step (sample_chain.cpp) -- the sampling update runs behind the logits tail in place of bio's beam update; tio: a
// device-chained timestamp step (ts_chain.cpp), the timestamp update in that place; tbio: a step of the beam search under the
// timestamp rules (tsbeam_chain.cpp), its two launches in that place.  At most one of bio / sio / tio / tbio is set.
struct StepCall {
  int k = 0, use_mask = 0;
  bool chained = false;
  int eot = -1, reps = 1;
  const BeamStepIO* bio = nullptr;
  const SampleStepIO* sio = nullptr;
  const TsStepIO* tio = nullptr;
  const TsBeamStepIO* tbio = nullptr;
};
constexpr uint64_t GRAPH_KEY_SAMPLE = 16u;   // bit of a captured step's key (launch_step): a sampling step
constexpr uint64_t GRAPH_KEY_TS = 32u;       // ... a timestamp step
constexpr uint64_t GRAPH_KEY_TSBEAM = 64u;   // ... a step of the beam search under the timestamp rules
// Launch one decode step: replay the captured graph for this launch shape (capturing it on first use), or enqueue the kernels
// eagerly.
int launch_step(wb_session* s, const StepPlan& plan, const StepCall& call);
// Range guard of the split-precision decoder GEMM: call wherever a decode has just synchronised with the host.
int dec_split_check(wb_session* s);

}  // namespace wb
