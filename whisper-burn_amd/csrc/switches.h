// Runtime switches: every WHISPER_HIP_* environment variable the library reads, in one table.  Each has one typed accessor in
// wb::sw; a switch is read ONCE per process, at the first call of its accessor (not when the library is loaded: a variable
// set before its path first runs takes effect).  switches.cpp is the only file that reads the environment.  INTEGRATION.md
// ("Runtime switches") lists the same rows.
#pragma once

namespace wb {
namespace sw {

// How a variable's value is read:
//   DEFAULT_ON  on unless the value starts with '0'
//   OPT_IN      on only if the value starts with '1'
//   UNSET_OR_1  on if unset or the value starts with '1' (any other set value: off)
//   TRI         unset: -1 (the built-in rule decides); value starts with '0': 0 (off); anything else: 1 (on)
//   INT         atoi of the value; the default when unset
//   STR         the value itself; nullptr when unset
enum Kind { DEFAULT_ON, OPT_IN, UNSET_OR_1, TRI, INT, STR };

// X(accessor, variable, kind, default, what it does)
#define WB_BOOL_SWITCHES(X)                                                                                                          \
  X(graph, "WHISPER_HIP_GRAPH", DEFAULT_ON, "on", "replay captured hipGraphs of the decode steps; 0: enqueue every step eagerly")    \
  X(chain, "WHISPER_HIP_CHAIN", DEFAULT_ON, "on", "device-chained greedy decode; 0: one host round trip per step")                   \
  X(beam_chain, "WHISPER_HIP_BEAM_CHAIN", DEFAULT_ON, "on", "beam bookkeeping on the device; 0: host-driven beam search")            \
  X(persist, "WHISPER_HIP_PERSIST", DEFAULT_ON, "on", "persistent flag-chained greedy kernel; 0: one launch per sublayer")           \
  X(persist_prefill, "WHISPER_HIP_PERSIST_PREFILL", DEFAULT_ON, "on", "the persistent launch runs the prompt itself; 0: host prefill") \
  X(prefill_pass, "WHISPER_HIP_PREFILL_PASS", DEFAULT_ON, "on", "a session's prefill mode 1 is honoured (one-pass prompt prefill); 0: steps everywhere") \
  X(poll, "WHISPER_HIP_POLL", DEFAULT_ON, "on", "chained greedy: spin on mapped progress flags; 0: copy + synchronise per chunk")    \
  X(speculate, "WHISPER_HIP_SPECULATE", OPT_IN, "off", "chained greedy: enqueue one segment ahead of the finished flags")            \
  X(fuse_sub, "WHISPER_HIP_FUSE_SUB", DEFAULT_ON, "on", "fused self-attention and MLP sublayer kernels; 0: per-matrix GEMVs")        \
  X(fuse_x, "WHISPER_HIP_FUSE_X", DEFAULT_ON, "on", "fused cross-attention sublayer kernel; 0: chunked cross-attention + GEMV")      \
  X(fuse_q, "WHISPER_HIP_FUSE_Q", DEFAULT_ON, "on", "chunked cross-attention blocks project their own queries")                      \
  X(fuse_co, "WHISPER_HIP_FUSE_CO", OPT_IN, "off", "chunked cross-attention blocks apply the out-projection too")                    \
  X(fuse16, "WHISPER_HIP_FUSE16", DEFAULT_ON, "on", "9 - 16 live rows stay on the fused sublayer kernels; 0: batch mode")            \
  X(batch_skinny, "WHISPER_HIP_BATCH_SKINNY", DEFAULT_ON, "on", "batch mode: skinny weight-stream GEMM up to 64 rows; 0: tiled GEMM") \
  X(cross_stream, "WHISPER_HIP_CROSS_STREAM", DEFAULT_ON, "on", "batch mode, one beam per window: streaming cross-attention")        \
  X(sk_pair, "WHISPER_HIP_SK_PAIR", OPT_IN, "off", "skinny GEMM: the waves' partial tiles meet pairwise")                            \
  X(mlp16_mfma, "WHISPER_HIP_MLP16_MFMA", DEFAULT_ON, "on", "9 - 16-row fused MLP on the matrix cores; 0: two row groups of 8")      \
  X(logits_mfma, "WHISPER_HIP_LOGITS_MFMA", DEFAULT_ON, "on", "9 - 16-row logits product on the matrix cores")                       \
  X(logits_preln, "WHISPER_HIP_LOGITS_PRELN", DEFAULT_ON, "on", "9 - 16-row logits: fold + LayerNorm once, in its own launch")       \
  X(logits_mr16, "WHISPER_HIP_LOGITS_MR16", DEFAULT_ON, "on", "9 - 16-row logits GEMV as one 16-row tile")                           \
  X(encoder_split, "WHISPER_HIP_ENCODER_SPLIT", UNSET_OR_1, "on", "split-precision (fp16 hi / lo) encoder-side GEMMs; 0: exact f32") \
  X(decoder_split, "WHISPER_HIP_DECODER_SPLIT", DEFAULT_ON, "on", "split-precision batch-mode decoder GEMM; 0: exact f32")           \
  X(encoder_pieces, "WHISPER_HIP_ENCODER_PIECES", DEFAULT_ON, "on", "encoder activations travel as fp16 pieces between split GEMMs") \
  X(attn_f16, "WHISPER_HIP_ATTN_F16", DEFAULT_ON, "on", "encoder attention on fp16 pieces; 0: the f32 kernels")                      \
  X(attn_kvsplit, "WHISPER_HIP_ATTN_KVSPLIT", DEFAULT_ON, "on", "encoder attention splits long key ranges across blocks")            \
  X(gpu_turn, "WHISPER_HIP_GPU_TURN", DEFAULT_ON, "on", "one entry point at a time per device and process (developer: 0 drops it)")  \
  X(session_pool, "WHISPER_HIP_SESSION_POOL", DEFAULT_ON, "on", "released sessions are parked for reuse; 0: freed (developer A/B)")  \
  X(pcm_stage, "WHISPER_HIP_PCM_STAGE", OPT_IN, "off", "host PCM is uploaded through a pinned per-session buffer")
#define WB_INT_SWITCHES(X)                                                                                                           \
  X(cross_stream_fuse, "WHISPER_HIP_CROSS_STREAM_FUSE", TRI, -1, "streaming cross-attention folds / projects its query; unset: d <= 768") \
  X(sk_max_blocks, "WHISPER_HIP_SK_MAX_BLOCKS", INT, 256, "skinny GEMM: most blocks a K-split may launch")                           \
  X(split_tile, "WHISPER_HIP_SPLIT_TILE", INT, 0, "split-precision GEMM: force a tile shape (developer A/B; 0: choose)")             \
  X(enc_trace_extra, "WHISPER_HIP_ENC_TRACE_EXTRA", INT, 0, "bit mask of extra stages in the encoder trace (1 pcm, 2 mel, 4 maxima)")
#define WB_STR_SWITCHES(X)                                                                                                           \
  X(enc_trace, "WHISPER_HIP_ENC_TRACE", STR, nullptr, "directory for per-thread dumps of the encoder stages (developer)")            \
  X(ps_stamps, "WHISPER_HIP_PS_STAMPS", STR, nullptr, "file for the persistent kernel's role timeline (developer)")                  \
  X(persist_resident, "WHISPER_HIP_PERSIST_RESIDENT", STR, nullptr, "persistent kernel: step-invariant operands stay in LDS (on); 0: off; log: on + report") \
  X(persist_setup, "WHISPER_HIP_PERSIST_SETUP", STR, nullptr, "persistent kernel: launch setup cached on the session (on); 0: built per call; log: on + report; 0log: both") \
  X(persist_deal, "WHISPER_HIP_PERSIST_DEAL", STR, nullptr, "persistent kernel: merge / final-LN roles kept off the first-layer attention blocks (on); legacy: the least loaded blocks; log: on + report") \
  X(persist_pick, "WHISPER_HIP_PERSIST_PICK", STR, nullptr, "persistent kernel: first-layer self-attention picks the next token from the tile records itself (on); merge: it waits for the merge role's row") \
  X(persist_mlp, "WHISPER_HIP_PERSIST_MLP", STR, nullptr, "persistent kernel: the MLP role publishes finished residual columns and the logits roles apply the final LayerNorm (on); planes: 4 d / 64 partial planes per layer and a final-LN role") \
  X(persist_inject_fail, "WHISPER_HIP_PERSIST_INJECT_FAIL", STR, nullptr, "test hook: \"launch\" = the cooperative launch is refused")

#define WB_SW_DECL(fn, name, kind, dflt, what) bool fn();
WB_BOOL_SWITCHES(WB_SW_DECL)
#undef WB_SW_DECL
#define WB_SW_DECL(fn, name, kind, dflt, what) int fn();
WB_INT_SWITCHES(WB_SW_DECL)
#undef WB_SW_DECL
#define WB_SW_DECL(fn, name, kind, dflt, what) const char* fn();
WB_STR_SWITCHES(WB_SW_DECL)
#undef WB_SW_DECL

}  // namespace sw
}  // namespace wb
