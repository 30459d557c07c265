/* prego_amd.h - C ABI of the MI355X-native PREGO step_recognition hot path.
 *
 * The reference (aleflabo/PREGO) is pure Python and has no FFI; its plug-in API for this path is the
 * string registry (step_recognition/utils/registry.py:6-20, model/model_builder.py:5-9).  The entry points
 * below are what a binding of that plug-in boundary needs; each one cites the reference interface it
 * replaces.  INTEGRATION.md shows the ctypes stub a PREGO maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only; no torch / HIP types in signatures
 *    (`prego_stream_t` is a `hipStream_t` passed as void*; NULL = the default stream).
 *  - every pointer called "device" is HBM memory of the current HIP device, fp32, row-major contiguous (the one exception: the
 *    inputs of prego_thumos_postprocess carry a row stride, ld_scores / ld_target, in elements).
 *  - functions return 0 on success, a negative PREGO_E* code otherwise; prego_last_error() gives the text.
 *  - calls only enqueue work on the caller's stream; nothing waits for the END of device work except prego_miniroad_check().  One
 *    documented wait for a START: a prego_miniroad_forward() that runs the split pass returns once the stream has reached its two
 *    persistent launches and they have confirmed each other resident (normally at once; behind earlier work of the stream otherwise).
 *  - the caller owns inputs, outputs, the workspace and the resident buffer (prego_miniroad_set_resident); they must stay valid until
 *    the stream reaches the end of the call.  The handle owns converted weight copies, the plan tables (pre-sized at create for clips
 *    of up to 131 072 frames: forward() allocates nothing below that; a longer clip or more clips than any call before grows them
 *    once, behind a stream synchronisation) and a pinned staging buffer for the per-call pointer tables (host pointer arrays passed
 *    to a call may be freed as soon as the call returns).  Nothing else is allocated by a hot call: every per-call buffer whose size
 *    depends on the call is the caller's, sized by a query (workspace_bytes, resident_bytes, backward_workspace_bytes).
 *  - one handle per (device, stream); different handles are independent and re-entrant.
 */
#ifndef PREGO_AMD_H
#define PREGO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: round 1.  2: round 2 entry points (step, adamw, vit, attention layer, window vote) and the grown forward workspace.
 * 3: round 3 (fp16 operand mode, device AP, window_vote marks windows with an id outside [0, n_classes) as -1).
 * 4: round 4 (PREGO_F16X2 split-operand mode; the prego_debug_* / _debug_stamps entry points left this header and the product library:
 *    prego_amd_debug.h / libprego_amd_debug.so).
 * 5: round 4, later (prego_miniroad_pass_info; the split pass behind prego_miniroad_forward).
 * 6: round 5.  Behaviour: a forward() that runs the split pass returns once its two launches have met - see prego_miniroad_forward -,
 *    a pass that cannot run side by side is re-run chunked inside the same call instead of being reported as PREGO_ETIMEOUT by
 *    prego_miniroad_check; tuning environment knobs are read by the debug library only.  Added (existing signatures unchanged):
 *    prego_miniroad_create_layers / _set_gru_layer (num_layers 2), prego_oad_loss_reduce (reduction 'sum'),
 *    prego_attention_layer_set_dropout, prego_perframe_ap_labels, prego_onehot_labels (host), prego_format_ids.
 * 7: round 6.  prego_miniroad_forward no longer allocates or synchronises for the whole-call relu(h) buffer: the caller sizes it with
 *    prego_miniroad_resident_bytes and hands it over with prego_miniroad_set_resident (without one, every call runs the chunked pass
 *    with the per-chunk classifier - same results).  Added: prego_miniroad_resident_bytes / _set_resident, prego_miniroad_guard_publish /
 *    _set_peer_guard (data-parallel training: a timeout on one rank stops the optimizer step of every rank), prego_miniroad_set_gru_layer_grads
 *    (training of a two-layer GRU; PREGO_FWD_KEEP now takes hidden_dim 512 / 1024 / 2048 and num_layers 1 / 2).  Existing signatures unchanged. */
#define PREGO_ABI_VERSION 7

enum {
  PREGO_OK = 0,
  PREGO_EINVAL = -1,       /* bad argument / unsupported dimension */
  PREGO_EHIP = -2,         /* a HIP runtime call failed */
  PREGO_EWORKSPACE = -3,   /* workspace too small */
  PREGO_ETIMEOUT = -4      /* the persistent recurrence kernel gave up waiting (reported by _check) */
};

/* MFMA operand type of a handle.  Accumulators, GRU state, gate math, LayerNorm statistics and softmax are fp32 in every mode.
 * PREGO_F16: IEEE fp16 operands and 16-bit intermediates - the same matrix rate and bytes as bf16 with 8x less operand rounding
 * (values beyond +-65504 saturate); inference entry points only (forward without PREGO_FWD_KEEP, step). */
enum { PREGO_F32 = 0, PREGO_BF16 = 1, PREGO_F16 = 2, PREGO_F16X2 = 3 };
/* PREGO_F16X2 ("fp16x2", round 4): split operands - every matrix operand travels as two fp16 numbers (hi + lo, ~22 mantissa bits) and
 * every product is three fp16 MFMA products with fp32 accumulation; intermediates, state and the classifier stay fp32.  The
 * argmax-identical mode of the north star (rnn.py:58-70: fp32-class results) at 3/16 of the matrix cost of PREGO_F32.  MiniROAD
 * inference entry point only (prego_miniroad_forward without PREGO_FWD_KEEP / PREGO_FWD_IN16). */

/* forward() flags */
enum {
  PREGO_FWD_SOFTMAX = 1,   /* eval branch of MROAD.forward: out = softmax(logits) (rnn.py:66-70); else raw logits */
  PREGO_FWD_KEEP = 2,      /* keep activations for backward() in the training workspace */
  PREGO_FWD_IN16 = 4       /* rgb[i] / flow[i] hold the handle's 16-bit operand type (bf16 or IEEE fp16 bits) instead of fp32: a feeder that
                            * keeps 16-bit features in pinned host memory ships half the bytes per frame; bf16 / fp16 handles, inference only */
};

typedef void* prego_stream_t;
typedef struct prego_miniroad prego_miniroad;

int prego_abi_version(void);
const char* prego_last_error(void);     /* most recent error text of the calling thread (any handle, or handle-free calls) */

/* ---- MiniROAD (MROAD, registry name "MiniROAD"): step_recognition/model/rnn/rnn.py:18-71 ---------------- */

/* MROAD.__init__ (rnn.py:21-49): d_rgb/d_flow = FEATURE_SIZES of cfg['rgb_type'/'flow_type'] (0 when
 * --no_rgb/--no_flow), emb = cfg['embedding_dim'], hid = cfg['hidden_dim'], n_classes = cfg['num_classes'].
 * Supported on gfx950: hid in {512, 1024, 2048} (see prego_miniroad_create_layers), emb % 512 == 0 (<= 4096), d_rgb % 64 == 0,
 * d_flow % 64 == 0, n_classes <= 128.  One GRU layer. */
int prego_miniroad_create(prego_miniroad** out, int d_rgb, int d_flow, int emb, int hid, int n_classes,
                          int compute_dtype);
/* The same with cfg['num_layers'] (rnn.py:32,38: nn.GRU(embedding_dim, hidden_dim, num_layers)): 1 or 2.  Hidden sizes (rnn.py:31): 512,
 * 1024, 2048 with 16-bit operands; 512, 1024 with PREGO_F32; 1024 with PREGO_F16X2 (the recurrence keeps its slice of W_hh in registers:
 * what does not fit is refused here with a message).  Two layers: PREGO_F32 / PREGO_BF16 / PREGO_F16.  Inference (forward without
 * PREGO_FWD_KEEP) covers all of these, and since ABI 7 so does training (PREGO_FWD_KEEP + prego_miniroad_backward; PREGO_BF16 / PREGO_F32
 * handles, hidden_dim 2048: PREGO_BF16; two layers: prego_miniroad_set_gru_layer_grads); prego_miniroad_step and the split pass stay with
 * hidden_dim 1024 / one layer. */
int prego_miniroad_create_layers(prego_miniroad** out, int d_rgb, int d_flow, int emb, int hid, int n_classes, int num_layers,
                                 int compute_dtype);
void prego_miniroad_destroy(prego_miniroad* h);
/* text of the last error raised by an entry point of THIS handle (handles are independent: one per (device, stream)) */
const char* prego_miniroad_last_error(const prego_miniroad* h);

/* load_state_dict (main.py:48): device fp32 tensors with the reference's state_dict shapes
 *   layer1.0.weight [emb, d_rgb+d_flow]  layer1.0.bias [emb]   layer1.1.weight/bias [emb]   (rnn.py:39-44)
 *   gru.weight_ih_l0 [3*hid, emb]  gru.weight_hh_l0 [3*hid, hid]  gru.bias_ih_l0/bias_hh_l0 [3*hid] (rnn.py:38)
 *   f_classification.0.weight [n_classes, hid]  f_classification.0.bias [n_classes]          (rnn.py:45-47)
 * The handle keeps its own (converted) copies: call again after every optimizer step. */
int prego_miniroad_set_weights(prego_miniroad* h, const float* layer1_w, const float* layer1_b, const float* ln_w,
                               const float* ln_b, const float* w_ih, const float* w_hh, const float* b_ih,
                               const float* b_hh, const float* fc_w, const float* fc_b, prego_stream_t stream);

/* Layer 1 of a two-layer handle (state_dict keys gru.weight_ih_l1 [3*hid, hid], gru.weight_hh_l1 [3*hid, hid], gru.bias_ih_l1,
 * gru.bias_hh_l1 [3*hid]); layer 0 comes with prego_miniroad_set_weights.  h0 / h_last of such a handle are [2][n_clips][hid]. */
int prego_miniroad_set_gru_layer(prego_miniroad* h, int layer, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                 prego_stream_t stream);

/* Largest number of clips one forward() call accepts (8192).  The call packs them, longest first, into its recurrence
 * slots (continuous batching: a slot runs several clips back to back, h restarts from 0 at every clip boundary), so
 * the number of sequential steps is max(longest clip, frames / slots).  Calls that pass h0 or h_last, or keep
 * activations for backward, need one clip per slot: at most 512 clips (bf16) / 256 (fp32). */
int prego_miniroad_max_clips(const prego_miniroad* h);

/* Workspace size (bytes) that lets forward() process `rows_per_chunk` packed rows (frames) per pipeline
 * pass; any size >= the value for rows_per_chunk = n_clips works, larger chunks run faster.
 * flags: PREGO_FWD_KEEP adds the activations backward() needs (whole batch resident). */
size_t prego_miniroad_workspace_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens,
                                      int64_t rows_per_chunk, int flags);

/* Whole-call resident buffer (ABI 7).  Long inference calls run the classifier ONCE behind the pass instead of once per chunk, and the
 * split pass (two persistent launches, prego_miniroad_pass_info) keeps its row map and counters beside it: both need relu(h) of every
 * frame of the call resident - 2 KB per frame with 16-bit operands, 4 KB with fp32 / fp16x2 operands (4.7 GB for a 2.3 M-frame eval
 * set).  resident_bytes: the size that lets a call of these clips and flags use those passes (0 = such a call never would: training
 * calls, num_layers 2, fewer than 65 536 frames, more than 24 GB).  set_resident: a device buffer (256-byte aligned) the handle may use
 * for this in every following forward() until it is replaced (NULL, 0 removes it); it is caller-owned, read and written only between the
 * start and the end of a forward() call in stream order, and holds nothing between calls.  A call whose size exceeds the registered
 * buffer simply runs the chunked pass with the per-chunk classifier: same result bits, ~20 % slower on the eval-set workload.
 * forward() itself never allocates device memory for it and never waits for the stream because of it. */
size_t prego_miniroad_resident_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens, int flags);
int prego_miniroad_set_resident(prego_miniroad* h, void* device_buffer, size_t bytes);

/* MROAD.forward (rnn.py:51-71) for a ragged batch, and the device half of Evaluate.eval (trainer/eval.py:36-56).
 *   lens[i]            frames of clip i (host array)
 *   rgb[i], flow[i]    device fp32 [lens[i], d_rgb] / [lens[i], d_flow]; flow == NULL or flow[i] == NULL means an
 *                      all-zero flow half (datasets/dataset.py:69) and skips its half of layer1's K dimension
 *   out[i]             device fp32 [lens[i], n_classes]: probabilities (PREGO_FWD_SOFTMAX) or logits; nullable
 *   argmax[i]          device int32 [lens[i]]: np.argmax(prob, axis=1) of eval.py:53, first max wins; nullable
 *   h0 / h_last        device fp32 [n_clips, hid] GRU state before frame 0 / after the last frame of each clip;
 *                      NULL h0 = zeros (rnn.py:49,60).  Chaining h_last -> h0 gives streaming inference.
 * The pointer arrays themselves are host arrays (copied during the call).
 * Which pass runs (prego_miniroad_pass_info reports it) is the library's choice per call and never changes a result bit.  The split pass
 * needs its two persistent launches resident together: they start with a bounded handshake, the call returns once it has succeeded, and
 * if it fails (a profiler that serialises kernel dispatches, another tenant holding the XCDs) both launches leave before either has
 * written anything and THIS call runs the chunked pass instead - no call is ever lost to the choice of pass. */
int prego_miniroad_forward(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* rgb,
                           const float* const* flow, float* const* out, int32_t* const* argmax, const float* h0,
                           float* h_last, int flags, void* workspace, size_t workspace_bytes,
                           prego_stream_t stream);

/* ---- MiniROADA (MROADA, registry name "MiniROADA"): step_recognition/model/rnn/rnn.py:73-136 ------------------------------------------
 * The MiniROAD trunk plus an anticipation head on every frame: A_l = relu(relu(h_t) W_a[l]^T + b_a[l]) for l < L, where W_a[l] is rows
 * l*hid .. l*hid + hid - 1 of anticipation_layer.0.weight (the .view(B, S, L, H) of rnn.py:125), and logits_l = A_l W_c^T + b_c with the SAME
 * f_classification weights as the frame's own logits (rnn.py:126).
 *
 * set_anticipation: load_state_dict of the head, device fp32 tensors with the reference's state_dict shapes
 *   anticipation_layer.0.weight [ant_len * hid, hid]   anticipation_layer.0.bias [ant_len * hid]
 * ant_len = cfg['anticipation_length'], 1..32.  The handle keeps converted copies (the handle's operand type): call again after the weights
 * change, like set_weights.  May allocate (and then synchronises `stream`) when ant_len grows.  Refused with a message on fp16x2 handles and
 * on num_layers 2 (the reference's own h0 is (1, B, H), rnn.py:122).  f_actionness is built by the reference but never used in forward. */
int prego_miniroad_set_anticipation(prego_miniroad* h, int ant_len, const float* w_a, const float* b_a, prego_stream_t stream);
/* MROADA.forward for a ragged batch: prego_miniroad_forward's arguments and behaviour (out / argmax are MROAD's logits / argmax, bit for bit
 * the same as prego_miniroad_forward's; h0 / h_last, passes, workspace_bytes / resident_bytes sizes, no device allocation, no host wait
 * beyond forward's) plus
 *   ant_out[i]       device fp32 [lens[i], ant_len, n_classes]: per-step probabilities (PREGO_FWD_SOFTMAX, rnn.py:131-134) or logits; nullable
 *   ant_argmax[i]    device int32 [lens[i], ant_len]: argmax over classes per step, first max wins; nullable
 * The head never materialises the [frames, ant_len * hid] intermediate; its sums are in a fixed order (repeat calls are bit-identical, and
 * which pass ran changes no bit).  Call set_anticipation first.
 * Training (PREGO_FWD_KEEP, bf16 / fp32 handles; fp16 / fp16x2 are refused, and so is PREGO_FWD_SOFTMAX with it): out and ant_out hold raw
 * logits (rnn.py:128-130).  Nothing beyond the trunk's kept activations is kept (the backward recomputes A_l with the forward's bits for the
 * rows that carry gradient), so workspace_bytes is the trunk's; the backward needs prego_miniroad_set_anticipation_grads. */
int prego_miniroad_forward_anticipation(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* rgb,
                                        const float* const* flow, float* const* out, int32_t* const* argmax,
                                        float* const* ant_out, int32_t* const* ant_argmax, const float* h0, float* h_last,
                                        int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);

/* Streaming inference, the online use of the model: ONE new frame for each of n_streams <= 16 independent streams -
 * MROAD.forward (rnn.py:51-71) with T = 1 and h0 = the state the previous call left.
 *   rgb / flow     device fp32 [n_streams, d_rgb] / [n_streams, d_flow], one frame per stream; flow == NULL = zero flow half
 *                  (rgb is ignored by a --no_rgb model)
 *   h_state        device fp32 [n_streams, hid], read and OVERWRITTEN with the new state (zeros before a stream's first frame)
 *   out            device fp32 [n_streams, n_classes]: probabilities (PREGO_FWD_SOFTMAX in flags) or logits; nullable
 *   argmax         device int32 [n_streams]; nullable
 * Three kernel launches for <= 4 streams (LayerNorm inside the W_ih product), four above; no plan, no workspace, no host staging (the general forward() with n_clips = 1, lens = {1}, h0, h_last is
 * the same arithmetic in eight launches plus table staging).  bf16 and fp16 handles (PREGO_EINVAL on fp32 / fp16x2 handles: use forward()).
 * Projection outputs stay fp32 here (forward()'s inference path rounds them to bf16), so the two paths agree to the operand
 * rounding, not bit for bit.  hidden_dim 1024, one GRU layer.  MiniROADA: prego_miniroad_step_anticipation below. */
int prego_miniroad_step(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out,
                        int32_t* argmax, int flags, prego_stream_t stream);
/* MiniROADA streaming - MROADA.forward (rnn.py:113-136) with T = 1 and h0 = the previous call's state: prego_miniroad_step plus
 *   ant_out        device fp32 [n_streams, ant_len, n_classes]: per-step probabilities (PREGO_FWD_SOFTMAX) or logits; nullable
 *   ant_argmax     device int32 [n_streams, ant_len]: first max wins; nullable
 * out, argmax and h_state are bit for bit prego_miniroad_step's (the same launches with the same arguments); the anticipation head follows
 * on the same stream in two more launches (csrc/stream_ant.hip) that read the new state, and none when both of its outputs are NULL.  Sums
 * in a fixed order: repeat calls are bit-identical.  No device allocation, no workspace, no host wait (set_anticipation holds the one
 * intermediate buffer, one per handle, as prego_miniroad_step's scratch: like every entry point of a handle, not to be called on one
 * handle from two streams at once).  prego_miniroad_step's refusals, and PREGO_EINVAL before set_anticipation. */
int prego_miniroad_step_anticipation(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state,
                                     float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags, prego_stream_t stream);
/* Wide streaming step: prego_miniroad_step / prego_miniroad_step_anticipation for 1 <= n_streams <= 256, the array shapes following
 * n_streams.  The weights cross the memory system once per call whatever n_streams is (csrc/stream_wide.hip): every product holds its weight
 * fragments in registers and walks the streams in tiles of 16, and the anticipation classifier takes 16 rows per workgroup.
 * Bits: a stream's out, argmax, new h_state, ant_out and ant_argmax are bit for bit what prego_miniroad_step (_anticipation) writes for that
 * stream in a call of 5..16 streams (every sum keeps that order), whatever n_streams is and wherever the stream stands in the call; repeat
 * calls are bit-identical.  With n_streams <= 16 the call IS prego_miniroad_step (_anticipation): its launches on the handle's own scratch
 * (the fused LayerNorm up to 4 streams included); the workspace may then be NULL and the query returns 0.
 *   workspace      device memory, 256-byte aligned, of at least prego_miniroad_step_wide_workspace_bytes(h, n_streams) bytes: the
 *                  intermediates that grow with the call (16-bit copies of the frame and the state, y, e, gi, gh and, once set_anticipation
 *                  has run, A [n_streams, ant_len * hid]; one size serves both entry points).  Query again after set_anticipation.
 * Every output is nullable as in prego_miniroad_step (_anticipation); with ant_out and ant_argmax both NULL the anticipation head is not
 * launched.  No device allocation, no host wait.  PREGO_EINVAL with a message, nothing written: n_streams outside 1..256, a NULL, unaligned
 * or too small workspace above 16 streams, everything prego_miniroad_step refuses, and _anticipation before set_anticipation. */
size_t prego_miniroad_step_wide_workspace_bytes(const prego_miniroad* h, int n_streams);
int prego_miniroad_step_wide(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state, float* out,
                             int32_t* argmax, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_miniroad_step_wide_anticipation(prego_miniroad* h, int n_streams, const float* rgb, const float* flow, float* h_state,
                                          float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags, void* workspace,
                                          size_t workspace_bytes, prego_stream_t stream);

/* Multi-frame streaming step (an addition to ABI 7, existing signatures unchanged): n_frames new frames for each of n_streams streams in ONE
 * call - a feeder that works in batches, a stream that reconnects with a backlog, a video that joins late.  1 <= n_frames <= 32, the same
 * for every stream of the call (ragged backlogs: prego_miniroad_step_ragged below), n_streams >= 1 and
 * n_streams * n_frames <= 256.  Longer backlogs, or more rows, are prego_miniroad_forward's work (h0 / h_last).
 *   rgb / flow     device fp32 [n_streams, n_frames, d_rgb] / [n_streams, n_frames, d_flow]; flow == NULL = zero flow half
 *   h_state        device fp32 [n_streams, hid], read and OVERWRITTEN with the state after the last frame
 *   out            device fp32 [n_streams, n_frames, n_classes]: probabilities (PREGO_FWD_SOFTMAX) or logits; nullable
 *   argmax         device int32 [n_streams, n_frames]; nullable
 *   ant_out        device fp32 [n_streams, n_frames, ant_len, n_classes]; nullable      ant_argmax  device int32 [n_streams, n_frames, ant_len]; nullable
 * Layer1, LayerNorm, the W_ih product, the classifier and the anticipation head do not depend on time: they run once over the
 * n_streams * n_frames rows with prego_miniroad_step_wide's kernels, their weights crossing the memory system once per call.  Only W_hh is on
 * the sequential path: one launch per frame that fuses gh = h W_hh^T with the GRU gates (csrc/stream_frames.hip), 5 + n_frames launches in
 * all (+ 2 for the anticipation head).
 * Bits: for every stream and every frame of the burst, out, argmax, ant_out, ant_argmax and the state after the frame are bit for bit what
 * prego_miniroad_step_wide (_anticipation) gives that stream driven frame by frame in calls of 5..256 streams - the unfused LayerNorm
 * route, at every n_streams: a call of <= 4 streams does NOT reproduce prego_miniroad_step's fused-LayerNorm bits.  They depend neither on
 * n_streams, n_frames nor on the stream's place in the call; repeat calls are bit-identical.
 *   workspace      device memory, 256-byte aligned, prego_miniroad_step_frames_workspace_bytes(h, n_streams, n_frames) bytes (0 = the
 *                  shape is refused): 16-bit frames, a copy of h_state, y, e, gi, the fp32 state after every frame, relu(h) rows and, once
 *                  set_anticipation has run, A [rows, ant_len * hid].  Query again after set_anticipation.
 * No device allocation, no host wait.  PREGO_EINVAL with a message, nothing launched: n_frames outside 1..32, n_streams * n_frames > 256,
 * a NULL, unaligned or too small workspace, everything prego_miniroad_step refuses, and _anticipation before set_anticipation. */
size_t prego_miniroad_step_frames_workspace_bytes(const prego_miniroad* h, int n_streams, int n_frames);
int prego_miniroad_step_frames(prego_miniroad* h, int n_streams, int n_frames, const float* rgb, const float* flow, float* h_state, float* out,
                               int32_t* argmax, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_miniroad_step_frames_anticipation(prego_miniroad* h, int n_streams, int n_frames, const float* rgb, const float* flow, float* h_state,
                                            float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags, void* workspace,
                                            size_t workspace_bytes, prego_stream_t stream);

/* Ragged streaming burst (an addition to ABI 7, existing signatures unchanged): prego_miniroad_step_frames with a frame count PER STREAM -
 * streams that reconnect with different backlogs, late joiners, a batching extractor that returns a different number of frames per video -
 * in ONE call instead of one call per group of equal backlog.
 *   n_frames       HOST int32 [n_streams], 1 <= n_frames[s] <= 32, R = sum n_frames[s] <= 256.  Read before the call returns and never
 *                  after: it may be freed or overwritten at once.  What the kernels need of it travels in their arguments.
 *   rgb / flow     device fp32, PACKED: [R, d_rgb] / [R, d_flow]; stream s owns rows off[s] .. off[s] + n_frames[s]) in frame order, off =
 *                  the prefix sum of n_frames in the caller's stream order; flow == NULL = zero flow half
 *   h_state        device fp32 [n_streams, hid], read and OVERWRITTEN: stream s is advanced by n_frames[s] frames
 *   out [R, n_classes], argmax [R], ant_out [R, ant_len, n_classes], ant_argmax [R, ant_len]: packed as the frames are; nullable as in
 *                  prego_miniroad_step_frames.  With every count equal to K this is byte for byte its [n_streams, K, ...] layout.
 * The launches are prego_miniroad_step_frames's over R rows, with one recurrent launch per frame index t = 0 .. max n_frames - 1 that
 * advances only the streams with n_frames[s] > t (csrc/stream_frames.hip: the streams are walked in descending order of count, so those
 * are a prefix): 5 + max n_frames launches (+ 2 for the anticipation head).
 * Bits: for every stream and frame, every output, the state after the frame and the state left in h_state are bit for bit
 * prego_miniroad_step_frames's (hence prego_miniroad_step_wide's frame by frame), whatever the other streams' counts, the order of the
 * streams in the call or the internal order.
 *   workspace      device memory, 256-byte aligned, prego_miniroad_step_ragged_workspace_bytes(h, n_streams, R) bytes (0 = the shape is
 *                  refused: n_streams outside 1..256, R < n_streams, R > 256); it depends on n_streams and R only.  Query again after
 *                  set_anticipation.
 * No device allocation, no host wait.  PREGO_EINVAL with a message, nothing launched: n_frames NULL, a count outside 1..32 (the message
 * names stream and count), R > 256, n_streams outside 1..256, a NULL, unaligned or too small workspace, everything prego_miniroad_step
 * refuses, and _anticipation before set_anticipation. */
size_t prego_miniroad_step_ragged_workspace_bytes(const prego_miniroad* h, int n_streams, int n_rows);
int prego_miniroad_step_ragged(prego_miniroad* h, int n_streams, const int32_t* n_frames, const float* rgb, const float* flow, float* h_state,
                               float* out, int32_t* argmax, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_miniroad_step_ragged_anticipation(prego_miniroad* h, int n_streams, const int32_t* n_frames, const float* rgb, const float* flow,
                                            float* h_state, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags,
                                            void* workspace, size_t workspace_bytes, prego_stream_t stream);

/* Stream pool (an addition to ABI 7, existing signatures unchanged): the online detector for a host whose streams open and close at
 * different times and of which only some have a new frame at any tick.  Every live video owns a SLOT of one device block: its GRU state
 * row (rnn.py:58-62 with h0 = the previous frame's state) and its running aggregation record - utils/aggregate.py:55-78 fed one id at a
 * time: the votes of the unfinished `window`-frame window and the list of (step id, first frame) events so far.  The pool object is host
 * memory (geometry, the addresses inside the caller's block); it owns no device memory.
 *   block           device memory, 256-byte aligned, at least prego_stream_pool_bytes(h, capacity, max_events) bytes, the caller's:
 *                   h [capacity][hid] fp32 at offset 0, then the records.  create enqueues its zeroing on `stream`; an all-zero slot is an
 *                   empty stream (zero state, no frames), so opening a stream needs no call.
 *   record of a slot (prego_stream_pool_record gives its address and size for ONE D2H copy), int32 words:
 *                   [0] frames  [1] last vote + 1 (0 = none yet)  [2] n_events  [3] overflow  [4 ..) counts[n_classes rounded up to 4]
 *                   event_id[max_events]  event_start[max_events]
 *                   aggregate.py:75-78's results follow as pred = event_id[0 .. n_events) and
 *                   changes_pred = event_start[1 .. n_events) + {frames} (after a flush; before it the last finished window ends at
 *                   frames - frames % window).
 *   update rule     one id of a slot: counts[id]++, frames++; when frames % window == 0 the window votes for the lowest id with the
 *                   maximal count (np.argmax(np.bincount(.)), aggregate.py:60), the counts are cleared, and when the vote differs from
 *                   the previous window's (or is the first) the event (vote, frame at which the window began) is appended.  A full
 *                   record sets bit 0 of overflow and drops the event (nothing is written past max_events); an id outside
 *                   [0, n_classes) sets bit 1 and counts nothing (np.bincount raises there; prego_window_vote marks it with -1).
 *   slots           HOST int32 [n]: which slots a call addresses, 1 <= n <= min(256, capacity), each in [0, capacity) and named once.
 *                   The list travels in the kernel arguments: it may be freed or reused as soon as the call returns.
 * prego_miniroad_step_pool: one new frame for the slots named, in three steps on `stream` - the slots' state rows are gathered into a dense
 * [n_active, hid] copy in the workspace, prego_miniroad_step_wide (_anticipation when ant_out or ant_argmax is non-NULL) runs on it
 * through its own entry point, the new rows go back to their slots and every slot's record takes its argmax.  rgb, flow, out, argmax,
 * ant_out, ant_argmax: dense, row i belongs to slots[i], with prego_miniroad_step_wide's shapes and nullability (a NULL argmax: the ids
 * go through the workspace).  Bits: a stream's outputs and its new state in the pool are bit for bit what prego_miniroad_step_wide writes
 * for a dense call of the same n_active streams; they depend neither on the slot numbers nor on the order of `slots` (the pool adds
 * no arithmetic).  Two launches more than prego_miniroad_step_wide; no device allocation, no host wait.
 *   workspace       device memory, 256-byte aligned, prego_miniroad_step_pool_workspace_bytes(h, n_active) bytes: the dense state, the
 *                   argmax vector and prego_miniroad_step_wide's workspace.  Query again after set_anticipation.
 * prego_stream_pool_vote: the record update alone, ids device int32 [n] from anywhere (the Transformer path, a general forward).
 * prego_stream_pool_flush: votes the unfinished window of each slot, the reference's shorter last window (aggregate.py:57-58); a slot
 * whose frames are a multiple of `window`, or that was flushed already, is left as it is.  prego_stream_pool_reset: zeroes state and record.
 * PREGO_EINVAL with a message, nothing launched: n outside 1..min(256, capacity), a slot outside [0, capacity), a slot named twice, a
 * NULL, unaligned or too small block or workspace, window < 1, max_events < 1, capacity or max_events above 1 048 576, a pool created for
 * another hidden size or class count, and everything prego_miniroad_step_wide refuses (fp32 / fp16x2 handles, hidden_dim != 1024, two
 * layers; ant_out / ant_argmax before set_anticipation).  A pool belongs to one stream at a time, as a handle does. */
typedef struct prego_stream_pool prego_stream_pool;
size_t prego_stream_pool_bytes(const prego_miniroad* h, int capacity, int max_events);
int prego_stream_pool_create(prego_stream_pool** out, const prego_miniroad* h, int capacity, int window, int max_events, void* device_block,
                             size_t bytes, prego_stream_t stream);
void prego_stream_pool_destroy(prego_stream_pool* p);
size_t prego_miniroad_step_pool_workspace_bytes(const prego_miniroad* h, int n_active);
int prego_miniroad_step_pool(prego_miniroad* h, prego_stream_pool* p, int n_active, const int32_t* slots, const float* rgb, const float* flow,
                             float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags, void* workspace,
                             size_t workspace_bytes, prego_stream_t stream);
/* prego_miniroad_step_pool for a burst: n_frames frames (1..32, n_active * n_frames <= 256) for each slot named - gather, then
 * prego_miniroad_step_frames (_anticipation when ant_out or ant_argmax is non-NULL) through its own entry point, then one commit that puts
 * every state row back once and has the slot's lane take the burst's n_frames ids in frame order, so a window may end inside the burst any
 * number of times; the overflow rules are the single-frame ones.  rgb, flow, out, argmax, ant_out, ant_argmax: dense with
 * prego_miniroad_step_frames's shapes, row i belongs to slots[i].  Bits: prego_miniroad_step_frames's; a slot's record afterwards is word
 * for word the record after n_frames prego_miniroad_step_pool calls.  A call that fails leaves the pool untouched.  Refusals:
 * prego_miniroad_step_pool's and prego_miniroad_step_frames's, nothing launched.  No device allocation, no host wait. */
size_t prego_miniroad_step_pool_frames_workspace_bytes(const prego_miniroad* h, int n_active, int n_frames);
int prego_miniroad_step_pool_frames(prego_miniroad* h, prego_stream_pool* p, int n_active, int n_frames, const int32_t* slots, const float* rgb,
                                    const float* flow, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax, int flags,
                                    void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* prego_miniroad_step_pool_frames with a frame count per slot: n_frames HOST int32 [n_active] (1..32 each, R = their sum <= 256; free to
 * reuse once the call returns, as `slots` is), frames and outputs packed as in prego_miniroad_step_ragged with row block i belonging to
 * slots[i] - gather, prego_miniroad_step_ragged (_anticipation when ant_out or ant_argmax is non-NULL) through its own entry point, then
 * one commit that puts every state row back once and has slot i's lane take its n_frames[i] ids in frame order.  Bits:
 * prego_miniroad_step_ragged's; a slot's record afterwards is word for word the record after n_frames[i] prego_miniroad_step_pool calls.
 * A call that fails leaves the pool untouched.  Refusals: prego_miniroad_step_pool's and prego_miniroad_step_ragged's, nothing launched.
 * Workspace: prego_miniroad_step_pool_ragged_workspace_bytes(h, n_active, R) bytes.  No device allocation, no host wait. */
size_t prego_miniroad_step_pool_ragged_workspace_bytes(const prego_miniroad* h, int n_active, int n_rows);
int prego_miniroad_step_pool_ragged(prego_miniroad* h, prego_stream_pool* p, int n_active, const int32_t* n_frames, const int32_t* slots,
                                    const float* rgb, const float* flow, float* out, int32_t* argmax, float* ant_out, int32_t* ant_argmax,
                                    int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_stream_pool_vote(prego_stream_pool* p, int n, const int32_t* slots, const int32_t* ids, prego_stream_t stream);
int prego_stream_pool_flush(prego_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream);
int prego_stream_pool_reset(prego_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream);
int prego_stream_pool_record(const prego_stream_pool* p, int slot, const void** device_record, size_t* bytes);

/* Synchronises `stream` and reports a recurrence timeout (PREGO_ETIMEOUT) or HIP error since the last check. */
int prego_miniroad_check(prego_miniroad* h, prego_stream_t stream);

/* Link-fed inference (the eval loop of trainer/eval.py:36-56 with features in host memory): let the H2D copy of a batch run UNDER its
 * forward instead of in front of it.
 *   plan_starts       the slot schedule the next forward of exactly these clips will use, costed for features that arrive at link speed
 *                     (link_row_bytes = bytes one frame moves over the link; 0 = features already in HBM): start_step[i] = the step at
 *                     which frame 0 of clip i is consumed, so frame a of clip i is needed at step start_step[i] + a; *n_steps = steps.
 *   set_feed_events   for the NEXT forward only: rows needed at steps < upto_step[j] are valid in the rgb / flow arrays once
 *                     events[0..j] (hipEvent_t recorded by the caller behind its copies, upto_step ascending) have fired; the last
 *                     upto_step must be >= *n_steps.  The library makes its packing stream wait for the events a chunk needs - the
 *                     caller copies in need order and never waits on the host.  Plain inference calls only (no h0 / h_last / KEEP). */
int prego_miniroad_plan_starts(prego_miniroad* h, int n_clips, const int32_t* lens, int link_row_bytes, int32_t* start_step, int32_t* n_steps);
int prego_miniroad_set_feed_events(prego_miniroad* h, int n_events, const int32_t* upto_step, void* const* events, int link_row_bytes);

/* Kernel-level timing hooks for bench.py's roofline leg: when enabled, forward() brackets its GEMM launches and
 * its recurrence launches with HIP events on the caller's stream; read() synchronises and returns the summed
 * milliseconds and launch counts since enable. */
int prego_miniroad_timing_enable(prego_miniroad* h, int enable);
/* (a split pass reports its recurrence launch in the gru slot and its feed-forward launch - pack, both projections, LayerNorm - in the
 * pack slot; gemm_flop still counts the projections' flops, gemm_ms / gemm_launches stay 0) */
int prego_miniroad_timing_read(prego_miniroad* h, double* gemm_ms, int64_t* gemm_launches, double* gemm_flop,
                               double* gru_ms, int64_t* gru_launches, double* pack_ms, int64_t* pack_launches,
                               double* pack_bytes);
/* What the last prego_miniroad_forward() of this handle ran (any pointer may be NULL): *mode = 0: the chunked pass (a chain of launches
 * per chunk); R > 0: the split pass - the recurrence of the whole call as ONE launch on R XCDs (16 R slots) beside ONE feed-forward
 * launch on the other XCDs (plain inference calls of 16-bit handles with >= 16 R clips and >= 262 144 frames, once an earlier
 * call has verified the workgroup placement; PREGO_SPLIT_PASS=R selects it).  *n_steps sequential recurrence steps, *n_slots slots. */
int prego_miniroad_pass_info(const prego_miniroad* h, int32_t* mode, int32_t* n_steps, int32_t* n_slots);

/* ---- training: trainer/train.py:6-29 (fwd, loss, backward); criterions/loss.py:15-34 -------------------------- */

/* nn.Dropout(p=cfg['dropout']) after layer1's ReLU (rnn.py:43): applied by forward() calls that carry
 * PREGO_FWD_KEEP (training mode); the mask is a stateless hash of (seed, element index), regenerated in backward. */
int prego_miniroad_set_dropout(prego_miniroad* h, float p, uint64_t seed);

/* OadLoss ("NONUNIFORM", loss.py:15-34): loss = mean_b sum_k -(y/||y||_2)_k * log_softmax(logits[b,-1,:])_k with
 * F.normalize's 1e-12 clamp.  logits[i], target[i]: device fp32 [lens[i], n_classes]; loss_out: device fp32 scalar;
 * dlogits[i] (array nullable): device fp32 [lens[i], n_classes] := grad_scale * dloss/dlogits (zero except last frame). */
int prego_oad_loss(int n_clips, const int32_t* lens, const float* const* logits, const float* const* target,
                   int n_classes, float* loss_out, float* const* dlogits, float grad_scale, prego_stream_t stream);
/* OadLoss(cfg, reduction) (loss.py:8-11,30-33): reduction 0 = 'mean' (what main.py builds; prego_oad_loss), 1 = 'sum' over the batch. */
int prego_oad_loss_reduce(int n_clips, const int32_t* lens, const float* const* logits, const float* const* target,
                          int n_classes, int reduction, float* loss_out, float* const* dlogits, float grad_scale, prego_stream_t stream);

/* loss.backward() through MROAD (train.py:23).  Must follow a forward() with PREGO_FWD_KEEP of the same clips whose
 * workspace is passed back as fwd_workspace (untouched in between).  dlogits[i]: device fp32 [lens[i], n_classes]
 * (any values: all frames are honoured).  The ten gradient tensors have the shapes of set_weights' arguments and are
 * OVERWRITTEN.  All column sums are fixed-order (deterministic). */
/* Data-parallel training (trainer/train.py:20-24 under clip sharding): hipEvent_t handles (NULL = none) that every following
 * prego_miniroad_backward records on its stream at two milestones - f_classification gradients final; all four GRU gradients
 * final - so the caller can all-reduce those buckets on another stream under the rest of the backward (layer1's weight gradient,
 * 47 % of the bytes, is final only when backward returns).  The events stay owned by the caller. */
int prego_miniroad_backward_events(prego_miniroad* h, void* ev_head_done, void* ev_gru_done);
/* Optional host callback of backward(): fn(user, bucket) is called on the calling thread, from inside prego_miniroad_backward, right after
 * the launches that make a group of gradient tensors final have been ENQUEUED and its event (above) recorded - bucket 0: f_classification,
 * bucket 1: the four GRU tensors.  A data-parallel caller enqueues that bucket's all-reduce there (behind the event, on its own
 * stream), i.e. ahead of the ~30 launches of the rest of the backward instead of behind them.  The callback must not call back into
 * this handle.  fn = NULL removes it. */
typedef void (*prego_bucket_fn)(void* user, int bucket);
int prego_miniroad_backward_callback(prego_miniroad* h, prego_bucket_fn fn, void* user);
/* A stacked GRU (num_layers 2, rnn.py:32,38) under loss.backward() (ABI 7): where the gradients of gru.weight_ih_l1 [3H, H],
 * gru.weight_hh_l1 [3H, H], gru.bias_ih_l1 [3H], gru.bias_hh_l1 [3H] go (device fp32, OVERWRITTEN by every following
 * prego_miniroad_backward; layer 0's are that call's own arguments).  Required before the backward of a 2-layer handle. */
int prego_miniroad_set_gru_layer_grads(prego_miniroad* h, int layer, float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh);
/* MiniROADA under loss.backward() (ABI 7 addition): what the NEXT prego_miniroad_backward takes for the anticipation head, after a
 * prego_miniroad_forward_anticipation with PREGO_FWD_KEEP (required then: that backward is refused without it; one backward only).
 *   d_ant[i]      device fp32 [lens[i], ant_len, n_classes]: the gradient of that forward's ant_out[i]; d_ant == NULL = zero gradient:
 *                 nothing of the head's backward runs, g_w_a / g_b_a are written as zeros and every other gradient is bit-identical to
 *                 MiniROAD's backward for the same dlogits
 *   g_w_a, g_b_a  device fp32 anticipation_layer.0.weight [ant_len * hid, hid] / .bias [ant_len * hid] gradients, OVERWRITTEN
 * The head's terms are added to g_fc_w / g_fc_b and to d relu(h) before the BPTT; g_w_a / g_b_a are final at the f_classification event
 * and callback (bucket 0).  The head's products touch only the span of packed rows that hold a non-zero d_ant value, found on the
 * device (no host wait); the backward workspace of a handle with set_anticipation holds the whole-range worst case. */
int prego_miniroad_set_anticipation_grads(prego_miniroad* h, const float* const* d_ant, float* g_w_a, float* g_b_a);
size_t prego_miniroad_backward_workspace_bytes(const prego_miniroad* h, int n_clips, const int32_t* lens);
int prego_miniroad_backward(prego_miniroad* h, int n_clips, const int32_t* lens, const float* const* dlogits,
                            float* g_layer1_w, float* g_layer1_b, float* g_ln_w, float* g_ln_b, float* g_w_ih,
                            float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_fc_w, float* g_fc_b,
                            void* fwd_workspace, size_t fwd_workspace_bytes, void* bwd_workspace,
                            size_t bwd_workspace_bytes, prego_stream_t stream);

/* utils/aggregate.py:55-72 on the device: the per-frame argmax of ONE video (device int32 [n_frames], as prego_miniroad_forward
 * writes it) is cut into consecutive windows of `window` frames (the reference uses 200; the last one may be shorter) and every
 * window votes for its most frequent class, the lowest class id winning a tie (np.argmax(np.bincount(.))).
 * votes: device int32 [ceil(n_frames / window)].  n_classes <= 128; a window that holds an id outside [0, n_classes) votes -1
 * (np.bincount raises on a negative id; the host wrapper turns the marker into an error).  The de-duplication / change lists of aggregate.py:75-78
 * then run over one value per window instead of one per frame. */
int prego_window_vote(const int32_t* argmax, int64_t n_frames, int window, int n_classes, int32_t* votes, prego_stream_t stream);

/* trainer/eval.py:59-65 writes the per-frame predicted and ground-truth class ids of every video as JSON text.  ids: device int32 [n]
 * (0 <= id <= 999); text: device uint32 [n], element i = the four bytes "%3d," of ids[i] in memory order (blanks in front of a number
 * are JSON whitespace), so the host cuts the text per video and turns every list's last comma into its bracket.  bad (nullable):
 * device int32, set to 1 when an id is out of range (its text is then "  0,": the caller must not use the text). */
int prego_format_ids(const int32_t* ids, int64_t n, uint32_t* text, int32_t* bad, prego_stream_t stream);

/* fp32 feature rows -> the 16-bit operand type, with the conversion the pack kernels apply (so a forward with
 * PREGO_FWD_IN16 on dst gives the bits of a forward on src).  n elements, n % 8 == 0; src, dst 16-byte aligned,
 * not overlapping; dtype PREGO_BF16 or PREGO_F16.  n == 0: nothing is launched.  Round to nearest even; PREGO_F16 saturates at
 * +-65504.  PREGO_EINVAL with a message, nothing launched: a NULL pointer, negative n, n % 8 != 0, a misaligned pointer, overlap, any
 * other dtype.  An addition to ABI 7 (existing signatures unchanged): what an evaluator that keeps its eval set in device memory
 * between calls converts its fp32 features with, once. */
int prego_cast_features(const float* src, void* dst, int64_t n, int dtype, prego_stream_t stream);

/* One training batch cut from a training set that stays in device memory: what the loader's default_collate stacks from the items of
 * datasets/dataset.py:96-132 (StepRecognitionDataset: rgb, flow, target of a window) or :138-231 (AnticipationDataset: also ant_target),
 * written by ONE launch on `stream`.  Allocates nothing, waits for nothing.  An addition to ABI 7 (existing signatures unchanged).
 *
 * Resident set, device memory: the UNPADDED videos one after the other - rgb_rows [n_rows][d_rgb] fp32, flow_rows [n_rows][d_flow] fp32
 * (NULL for a dataset without flow; flow_out is then NULL as well), and EITHER labels int32 [n_rows] (the row's class id, -1 for an
 * all-zero row: target rows are built as zeros with 1.0f at the class) OR dense_targets [n_rows][n_classes] fp32 (rows are copied).
 * vid_row0 int64 [n_videos]: a video's first resident row; vid_len int32 [n_videos]: its frames.
 *
 * Windows, device memory: table int32 [n_windows][2] = (video index, start row) per window, the start in the datasets' PADDED
 * coordinates (window_size - 1 zero rows in front of every video, dataset.py:53-55); bit 31 of the video word marks a PAD entry
 * (features of the window, all-zero target and ant_target).  order int32 [n_order]: indices into table in the order the sampler drew them;
 * the batch is order[first .. first + n).
 *
 * Outputs, device fp32 contiguous, each nullable: rgb_out [n][window_size][d_rgb], flow_out [n][window_size][d_flow],
 * target_out [n][window_size][n_classes], ant_target_out [n][ant_len][n_classes].
 *
 * Row rule: row r of a window with start s is padded row p = s + r of its video; ant_target row l is padded row p = s + window_size + l.
 * p < window_size - 1 or p >= vid_len[v] + window_size - 1 gives a row of zeros (nothing is read), every other p reads resident row
 * vid_row0[v] + p - (window_size - 1).  No table content makes the kernel read outside the resident arrays: an order entry outside
 * [0, n_windows), a video index outside [0, n_videos) or a resident row outside [0, n_rows) gives zeros.
 *
 * PREGO_EINVAL with a message, nothing launched: d_rgb or d_flow not a multiple of 4; rgb_rows, flow_rows or an output not 16-byte
 * aligned (a table not aligned to its element); n < 1; both or neither of labels / dense_targets; window_size < 1; ant_len < 0;
 * ant_target_out with ant_len == 0; an output without its resident rows; a NULL table; n_classes < 1; first / n outside order; a batch
 * of 2^31 or more rows or target elements. */
int prego_gather_windows(const float* rgb_rows, const float* flow_rows, int64_t n_rows, int d_rgb, int d_flow, const int32_t* labels,
                         const float* dense_targets, const int64_t* vid_row0, const int32_t* vid_len, int n_videos, const int32_t* table,
                         int n_windows, const int32_t* order, int64_t n_order, int64_t first, int n, int window_size, int n_classes,
                         int ant_len, float* rgb_out, float* flow_out, float* target_out, float* ant_target_out, prego_stream_t stream);

/* utils/metrics.py:25-62 on the device: sklearn.metrics.average_precision_score of every class column of the per-frame score
 * matrix the eval loop collects (trainer/eval.py:48-57; main.py:101 runs it after every epoch).  scores / target: device fp32
 * [n_frames][n_classes] row-major (target != 0 marks a positive).  Thresholds are the distinct score values (ties share one),
 * AP = sum_k (R_k - R_{k-1}) P_k.  ap: device double [n_classes] (NaN for a class without positives); n_pos (nullable): device
 * int64 [n_classes] positives per class; score_sum (nullable): device double [n_classes] column sums of the scores (the "pred:"
 * figure of metrics.py:52).  The caller applies the reference's "ignore class 0" rule (metrics.py:44-48) when averaging.
 * Exact integer ranks, fp64 sum: only thresholds that hold a positive contribute, so the positives of every class are sorted
 * (segmented radix sort) and every score is counted against them (csrc/metrics.hip).  Workspace:
 * prego_perframe_ap_workspace_bytes (16 B per score + histograms). */
size_t prego_perframe_ap_workspace_bytes(int64_t n_frames, int n_classes);
int prego_perframe_ap(const float* scores, const float* target, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                      double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* The same metric with the positives given as ONE class id per frame (device int32 [n_frames]; an id outside [0, n_classes) = a
 * frame without a positive): what a one-hot target matrix says, in 4 bytes per frame instead of 4 x n_classes.  Same results, bit for bit. */
int prego_perframe_ap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                             double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* utils/metrics.py:64-130 on the device with metrics='AP': average precision by tenth of each action (how early inside a step it is
 * recognised).  scores: device fp32 [n_frames][n_classes]; labels: device int32 [n_frames], one class id per frame in evaluation
 * order (an id outside [0, n_classes) = a frame that is a negative of every class).  Per class c the instances are the maximal runs
 * of labels == c over the whole axis (videos concatenated: a run is not cut at a video boundary); a run with first frame a and last
 * frame b has len = b - a and its stage s = 0..9 holds the frames [lo, hi), lo = a + trunc(len * (s / 10.0)),
 * hi = max(lo + 1, a + trunc(len * ((s + 1) / 10.0))) - IEEE double products, as the reference's int(len * perc) (len 90, s 7: offset
 * 62); a one-frame run is in all ten stages, the last frame of a longer run in none.  ap[s][c] is sklearn's average_precision_score
 * over the frames with labels != c (negatives) plus the stage-s frames of every run of c (positives): thresholds at the distinct
 * score values, ties share one, -0.0 == +0.0.  ap: device double [10][n_classes], 0.0 for a class without a run (what the reference
 * reports and averages); n_pos (nullable): device int64 [10][n_classes], the positives of each set.  Every class is computed; the
 * caller applies the "ignore class 0" rule.  Exact integer ranks, one fp64 sum per (stage, class) in a fixed order: the same bits on
 * every run; nothing returns to the host between the launches and nothing is allocated.  Workspace:
 * prego_perstage_ap_workspace_bytes (that of prego_perframe_ap + 40 B per frame, whatever the run lengths).  n_frames == 0: returns
 * 0 and writes 0.0 / 0.  PREGO_EINVAL, checked before any launch (outputs and workspace untouched): a NULL scores, labels or ap, a
 * NULL workspace with n_frames > 0, n_frames < 0 or >= 2^31, n_classes < 1 or > 65535; PREGO_EWORKSPACE: workspace_bytes below the
 * query.  An addition to ABI 7 (existing signatures unchanged).  Dense multi-label targets: the host path (prego_amd/metrics.py). */
size_t prego_perstage_ap_workspace_bytes(int64_t n_frames, int n_classes);
int prego_perstage_ap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                             void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* utils/metrics.py:10-22 on the device: the calibrated average precision (metric 'cAP', the TVSeries metric) of every class column,
 * beside prego_perframe_ap with the same arguments.  The order is descending score, frames of equal score by ascending frame index
 * (-0.0 == +0.0): the reference's unstable argsort leaves ties to chance, this is the order of the host form
 * (prego_amd.metrics.calibrated_average_precision_columns).  With q_0 .. q_{P-1} the class's positives in that order and rank_i the
 * 1-based position of q_i among all n frames:  tps_i = i + 1, fps_i = rank_i - tps_i, w = (n - P) / P, eps = 2^-52,
 *   cAP = (1 / P) * sum_i tps_i / (tps_i + fps_i / (w + eps) + eps)      in IEEE double, in this operand order.
 * ap: device double [n_classes] (NaN for a class without positives); n_pos / score_sum (nullable) as prego_perframe_ap.  Exact integer
 * ranks (the positives sorted by (score key, frame), every (score, frame) counted against them), one fp64 sum per class in a fixed
 * order: the same bits on every run.  Workspace: prego_perframe_cap_workspace_bytes (24 B per score + histograms).  n_frames == 0:
 * returns 0, writes NaN / 0 / 0.0 and needs no workspace.  PREGO_EINVAL, checked before any launch (outputs and workspace untouched):
 * a NULL scores, target / labels or ap, a NULL workspace with n_frames > 0, n_frames < 0 or >= 2^31, n_classes < 1 or > 65535;
 * PREGO_EWORKSPACE: workspace_bytes below the query.  An addition to ABI 7 (existing signatures unchanged). */
size_t prego_perframe_cap_workspace_bytes(int64_t n_frames, int n_classes);
int prego_perframe_cap(const float* scores, const float* target, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                       double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* The same with one class id per frame, as prego_perframe_ap_labels: bit for bit the results of one-hot target rows. */
int prego_perframe_cap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                              double* score_sum, void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* utils/metrics.py:64-130 with metrics='cAP' (the reference's default there): prego_perstage_ap_labels' sample sets - the negatives of
 * class c plus the stage-s frames of its runs - under the calibrated metric and the order above.  For a stage member q_i of class c:
 * tps = the stage members among q_0 .. q_i, fps = rank_i - (i + 1) (the negatives in front of q_i, the same in every stage),
 * w = (n - P_c) / P_cs, the sum divided by P_cs = the stage's members.  ap: device double [10][n_classes], NaN where a (stage, class)
 * has no member (what the host's perstage_ap_raw(.., 'cAP') answers); n_pos (nullable): device int64 [10][n_classes].  Workspace:
 * prego_perstage_cap_workspace_bytes (that of prego_perframe_cap + 40 B per frame).  n_frames == 0: returns 0 and writes 0.0 / 0, as
 * prego_perstage_ap_labels.  Refusals as prego_perstage_ap_labels.  An addition to ABI 7. */
size_t prego_perstage_cap_workspace_bytes(int64_t n_frames, int n_classes);
int prego_perstage_cap_labels(const float* scores, const int32_t* labels, int64_t n_frames, int n_classes, double* ap, int64_t* n_pos,
                              void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* utils/postprocessing.py:4-29 on the device: what the reference applies in front of every metric when the data set is THUMOS.
 * scores: device fp32, n_frames rows of n_classes values, row stride ld_scores ELEMENTS (>= n_classes; step l of an [n][L][C] tensor is
 * scores + l C with ld_scores = L C, no copy); target: the same with ld_target, or labels: device int32 [n_frames], one class id per frame.
 * In the reference's order:
 *   1. PREGO_THUMOS_SMOOTH: s'[i][c] = max over d in (0, -1, +1, -2, +2) of s[j][c], j = i + d if 0 <= i + d < n_frames, else j = i -
 *      bit for bit the reference's five shifted copies for n_frames >= 2; for n_frames == 1 (where the reference's np.squeeze drops
 *      the frame axis and its result is ill-defined) it is DEFINED by this formula: the row itself.  It runs over the whole matrix
 *      before any row is removed, across video boundaries, as the reference does.  max is np.maximum: a NaN propagates.
 *   2. PREGO_THUMOS_SWITCH: s'[i][switch_to] = s'[i][switch_from] where that is greater (5 and 8 in the reference), after smoothing.
 *   3. row i is kept iff target[i][ambiguous] != 1.0f exactly (a 0.5 keeps the row) / labels[i] != ambiguous (21 in the reference;
 *      -1: every row is kept).  The kept rows of s' and of target / labels are written to scores_out / target_out (dense, row stride
 *      n_classes) / labels_out in frame order; *n_valid (device int64) = their number.  The outputs must hold n_frames rows; rows from
 *      *n_valid on are not written, kept rows are written once, the inputs are never written.
 * Only comparisons and copies, a block-wise count, a scan of the counts and a scatter (no atomics): the same bits as the reference, on
 * every run.  The scores are read from HBM once: a smoothing tile of PREGO_THUMOS_TILE_ROWS rows is staged in LDS with two rows above
 * and below it.  Everything is enqueued on `stream`; nothing is allocated, nothing waits.  Workspace:
 * prego_thumos_postprocess_workspace_bytes (4 B per tile).  n_frames == 0: returns 0, writes *n_valid = 0, needs no workspace.
 * PREGO_EINVAL, checked before any launch (outputs, *n_valid and workspace untouched): a NULL input or output (a NULL workspace with
 * n_frames > 0), a pointer not aligned to its element, n_frames < 0 or >= 2^31, n_classes outside 1 .. 65535, unknown flag bits,
 * ld_scores / ld_target < n_classes, ambiguous < -1 or >= n_classes, with PREGO_THUMOS_SWITCH a switch column outside [0, n_classes)
 * or switch_from == switch_to, an output (or the workspace) that overlaps an input; PREGO_EWORKSPACE: workspace_bytes below the query.
 * An addition to ABI 7 (existing signatures unchanged). */
enum { PREGO_THUMOS_SMOOTH = 1, PREGO_THUMOS_SWITCH = 2 };
#define PREGO_THUMOS_TILE_ROWS 128
size_t prego_thumos_postprocess_workspace_bytes(int64_t n_frames, int n_classes);
int prego_thumos_postprocess(const float* scores, int64_t ld_scores, const float* target, int64_t ld_target, int64_t n_frames, int n_classes,
                             int flags, int switch_from, int switch_to, int ambiguous, float* scores_out, float* target_out,
                             int64_t* n_valid, void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_thumos_postprocess_labels(const float* scores, int64_t ld_scores, const int32_t* labels, int64_t n_frames, int n_classes, int flags,
                                    int switch_from, int switch_to, int ambiguous, float* scores_out, int32_t* labels_out, int64_t* n_valid,
                                    void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* Segmental metrics on the device: what step-recognition results on Assembly101 are reported in - frame accuracy (MoF), segmental
 * Edit score and segmental F1 at three overlaps - from the transcripts that one class id per frame spells out.
 * INPUTS.  pred / gt: device int32 [n_frames], one id per frame, n_videos videos one after the other; offsets: device int32
 * [n_videos + 1], video v owns the frames [offsets[v], offsets[v + 1]).  Every word of offsets is clamped into [0, n_frames] before it
 * indexes memory and a descending pair is an empty video; the records are defined for ascending offsets (videos that overlap share
 * workspace: their records are unspecified, nothing is read or written out of bounds).  bg_mask: HOST, 128 bits, bit c set = class c
 * is background (NULL = no background class, PREGO's data sets).  overlap_num / overlap_den: HOST, three overlaps as rationals,
 * 0 < num <= den <= 32768 (both NULL = 1/10, 1/4, 1/2).
 * SEGMENTS of a label sequence of ONE video: the maximal runs of equal id inside that video, in frame order - a run never continues
 * across a video boundary (prego_perstage_ap_labels does the opposite).  Runs whose id is in [0, 128) and set in the mask are dropped;
 * two runs of one id separated only by a dropped run stay two segments.  A segment is (id, start, end), end exclusive.  Ids outside
 * [0, 128) are ordinary ids, compared for equality only, never background.  m, n: the pred and gt segments of the video.
 * PER VIDEO.  correct = frames with pred == gt, frames = its length (background frames count in both).  dist = the Levenshtein
 * distance of the two segment-id lists (insert, delete, substitute 1; match 0).  For a pred segment p and a gt segment g of the same
 * id: inter = min(pe, ge) - max(ps, gs), union = max(pe, ge) - min(ps, gs); the candidates of p are the same-id gt segments with
 * inter > 0, best(p) the candidate with the largest inter / union (64-bit cross products; equal ratios: the earliest gt segment);
 * p qualifies at k when inter * den_k >= union * num_k.  tp_k = the gt segments g for which some pred segment has best(p) = g and
 * qualifies at k; fp_k = m - tp_k, fn_k = n - tp_k.  (The usual sequential rule without its order: walk the pred segments, take the
 * argmax of IoU x id equality over the gt segments, a true positive if the IoU reaches the overlap and that gt segment is not hit
 * yet.  Below 2^31 frames two distinct ratios, or a ratio and a threshold, differ by at least 1 / (10 * 2^31): the rational compares
 * agree with that formulation's fp64 divisions.)
 * RECORD.  records: device int32 [n_videos][8], 16-byte aligned:  correct | frames | m | n | dist | tp_0 | tp_1 | tp_2.
 * REPORT (the caller's, fp64, in this operand order): MoF = 100 * sum(correct) / sum(frames) (0.0 without frames); Edit = the mean over
 * the videos of 100 * (1 - dist / max(m, n, 1)); F1@k = 200 * TP_k / (M + N) over the sums of tp_k, m, n (0.0 when M + N == 0).
 * One launch, one workgroup per video (csrc/segmental.hip): frame scan and compaction, the Levenshtein table by anti-diagonals - three
 * diagonals of min(m, n) + 1 ints in LDS while min(m, n) <= PREGO_SEGMENTAL_LDS_SEGMENTS, in the workspace above it (slow; no video
 * is refused for its size) -, a bisection per pred segment.  Integers only: the same words on every run.  Everything is enqueued on
 * `stream`; nothing is allocated, nothing waits.  Workspace: prego_segmental_workspace_bytes (40 B per frame + 12 B per video).
 * n_frames == 0: returns 0, every record is eight zeros, no workspace is needed.  PREGO_EINVAL, decided before the launch (records
 * and workspace untouched): a NULL pred, gt, offsets or records, a NULL workspace with n_frames > 0, n_videos < 1, n_frames < 0 or
 * >= 2^31, records not 16-byte aligned, only one of overlap_num / overlap_den, an overlap outside 0 < num <= den <= 32768;
 * PREGO_EWORKSPACE: workspace_bytes below the query.  An addition to ABI 7 (existing signatures unchanged). */
#define PREGO_SEGMENTAL_LDS_SEGMENTS 2047
size_t prego_segmental_workspace_bytes(int64_t n_frames, int n_videos);
int prego_segmental_scores(const int32_t* pred, const int32_t* gt, const int32_t* offsets, int n_videos, int64_t n_frames,
                           const uint32_t bg_mask[4], const int32_t overlap_num[3], const int32_t overlap_den[3], int32_t* records,
                           void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* Viterbi decoding on the device: the cheapest label sequence of every video under per-frame emission costs and a first-order
 * transition matrix - the smoother Edit / F1 on Assembly101 are reported with.  Everything is integer: the same words come out on
 * every run, and the device and the host model (prego_amd/decode.py) agree to the bit.
 * UNITS.  Costs are in 1/256 bit: 256 units = a factor 2 in probability.  PREGO_DECODE_CAP = 32767.  PREGO_DECODE_FORBIDDEN = -1.
 * EMISSION COST OF A PROBABILITY.  Take the fp32 word of p.  No log2f is used, so host and device cannot differ.
 *   - If the sign bit is set, p is NaN, or the exponent field E is 0 (zero or denormal): cost = CAP.
 *   - If p >= 1.0f (+inf included): cost = 0.
 *   - Otherwise E is in 1..126 and k = mantissa >> 15 is in 0..255: cost = 256 * (127 - E) - LUT[k], with
 *     LUT[k] = rint(256 * log2(1 + (k + 0.5) / 256)).
 *   - The largest value is 256 * 126 - LUT[0] = 32255, so CAP only marks non-positive and denormal inputs.
 * LUT is a table of 256 literals, present once on the host (prego_amd/decode.py) and once for the kernels (csrc/decode_model.h).  The closest
 * any of the 256 values comes to a rounding tie is 1.6e-3 (k = 118), so the table is the same under any libm.
 * MODEL.  C classes, 1 <= C <= 128.  trans: int32 [C][C]; trans[i][j] is the cost of label i at frame t-1 followed by j at frame t.  A
 * negative word is FORBIDDEN.  A word above CAP is read as CAP.  init: int32 [C] or NULL (= zeros), with the same clamping.
 * PER VIDEO (frames [offsets[v], offsets[v+1]), clamped exactly as in prego_segmental_scores: every word of offsets into
 * [0, n_frames], a descending pair is an empty video; videos that overlap share workspace and labels: their results are unspecified,
 * nothing is read or written out of bounds).  Here e_t(j) is the emission cost of frame t and class j.
 *   - d_0(j) = init[j] + e_0(j), or INFINITE if init[j] is forbidden.
 *   - d_t(j) = e_t(j) + min over i with trans[i][j] allowed and d_{t-1}(i) finite of (d_{t-1}(i) + trans[i][j]).  The back-pointer is
 *     the LOWEST i that attains the minimum.  With no such i, d_t(j) is INFINITE.
 *   - End state: the lowest j with the minimal finite d_{T-1}(j).
 *   - The labels are the back-pointer chain.
 *   - If every state is INFINITE at some frame the video is infeasible: all its labels are -1 and its record is -1 | -1.
 *   - An empty video has record 0 | -1.
 * RECORD.  records: device int64 [n_videos][2], 16-byte aligned:  total cost | end state.  labels: device int32 [n_frames].
 * EXACTNESS.  d is exact for every accepted input: 64-bit accumulators (a finite d reaches n_frames * 65534, which passes 2^31 beyond
 * 32769 frames); no state is saturated, however far above the step's minimum it is - it may be the only one with an allowed
 * continuation.  (Stretches of at most PREGO_DECODE_BLOCK steps at whose start every finite d lies within 2^24 - 64 * 65534 of the
 * smallest run on 32-bit values relative to it; csrc/decode.hip carries the proof that they cannot overflow.  The others run in 64 bits.)
 * INPUTS.  prego_viterbi_decode: probs device fp32 [n_frames][ld], quantised on load by the rule above.  prego_viterbi_decode_costs:
 * costs device int32 [n_frames][ld], every word clamped into [0, CAP] on load.  prego_emission_costs: probs [n_frames][ld] -> costs
 * int32 [n_frames][n_classes] (dense rows) by the same quantiser; decoding its output equals decoding the probabilities.
 * One launch, one 256-thread workgroup per video (csrc/decode.hip): the forward pass keeps a column slice of trans in registers and
 * d_{t-1} in LDS, one barrier per step, emission rows requested PREGO_DECODE_PREFETCH frames ahead, one back-pointer byte per
 * (frame, class) to the workspace; the backtrace cuts the video into blocks of PREGO_DECODE_BLOCK frames: every block's end -> start
 * map in parallel, the maps composed in LDS, every block walked once more from its known end state.  Everything is enqueued on
 * `stream`; nothing is allocated, nothing waits.  Workspace: prego_viterbi_workspace_bytes (n_classes bytes per frame and per block).
 * n_frames == 0: returns 0, every record is 0 | -1, no workspace is needed.  PREGO_EINVAL, decided before any launch (labels,
 * records and workspace untouched): a NULL probs / costs, offsets, trans, labels or records, a NULL workspace with n_frames > 0,
 * n_videos < 1, n_frames < 0 or >= 2^31, n_classes outside 1..128, ld < n_classes, records not 16-byte aligned, labels, records or
 * workspace overlapping an input (or, prego_emission_costs, costs overlapping probs).  PREGO_EWORKSPACE: workspace_bytes below the
 * query.  An addition to ABI 7 (existing signatures unchanged). */
#define PREGO_DECODE_CAP 32767
#define PREGO_DECODE_FORBIDDEN (-1)
#define PREGO_DECODE_MAX_CLASSES 128
#define PREGO_DECODE_BLOCK 64
#define PREGO_DECODE_PREFETCH 8
size_t prego_viterbi_workspace_bytes(int64_t n_frames, int n_videos, int n_classes);
int prego_viterbi_decode(const float* probs, int64_t ld, const int32_t* offsets, int n_videos, int64_t n_frames, int n_classes,
                         const int32_t* trans, const int32_t* init, int32_t* labels, int64_t* records, void* workspace,
                         size_t workspace_bytes, prego_stream_t stream);
int prego_viterbi_decode_costs(const int32_t* costs, int64_t ld, const int32_t* offsets, int n_videos, int64_t n_frames, int n_classes,
                               const int32_t* trans, const int32_t* init, int32_t* labels, int64_t* records, void* workspace,
                               size_t workspace_bytes, prego_stream_t stream);
int prego_emission_costs(const float* probs, int64_t ld, int64_t n_frames, int n_classes, int32_t* costs, prego_stream_t stream);
/* HOST function (no device work): the reference's loader yields fp32 target rows [n_frames][n_classes] per video (one-hot for both
 * shipped configs).  targets: n_videos host pointers, n_frames: their row counts; labels: host int32 [sum of n_frames], the videos one
 * after the other, labels[i] = np.argmax(row i) (eval.py:55, the first maximum); onehot[v] = 1 iff every row of video v holds exactly one
 * nonzero entry and it is positive - then the labels say everything the matrix does and prego_perframe_ap_labels replaces
 * prego_perframe_ap (the eval loop sends 4 bytes per frame over the link instead of 4 x n_classes).  Up to 16 threads. */
int prego_onehot_labels(int n_videos, const float* const* targets, const int64_t* n_frames, int n_classes, int32_t* labels,
                        int32_t* onehot);

/* torch.optim.AdamW as main.py:62-67 builds it (amsgrad off, maximize off), fused over a tensor list in one launch:
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * params/grads/exp_avg/exp_avg_sq: host arrays of n_tensors device fp32 pointers; numel: host array; step is 1-based. */
int prego_adamw_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                     float* const* exp_avg_sq, const int64_t* numel, int64_t step, float lr, float beta1, float beta2, float eps,
                     float weight_decay, prego_stream_t stream);
/* The same step for MiniROAD's ten tensors (prego_miniroad_set_weights' order, reference state_dict shapes) that ALSO rewrites the
 * handle's converted operand copies from the updated values in the same pass: the training loop (train.py:24 optimizer.step())
 * needs no prego_miniroad_set_weights after it.  The launch is GUARDED by the handle's timeout word on the device: while a recurrence /
 * BPTT timeout of this handle is pending (set by the kernel that gave up, cleared by prego_miniroad_check, which reports it), the step
 * changes nothing - a training loop may enqueue it without synchronising first and still never applies garbage gradients. */
int prego_miniroad_adamw_step(prego_miniroad* h, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float eps,
                              float weight_decay, prego_stream_t stream);
/* The same guard across data-parallel ranks (ABI 7; train.py:20-24 under clip sharding).  A rank whose kernels gave up still takes part
 * in the gradient all-reduce, so its garbage reaches every rank: the guard has to be collective.
 *   guard_publish: enqueue dst[0] = (this handle's timeout word is set) ? 1.0f : 0.0f.  dst is one fp32 element of the gradient bucket
 *                  the ranks sum (the caller reserves it; call it after prego_miniroad_backward, before that bucket's all-reduce).
 *   set_peer_guard: the address of that element (after the reduction it is non-zero iff ANY rank gave up), NULL = none.  While it
 *                  holds a non-zero value prego_miniroad_adamw_step changes nothing AND raises this handle's own timeout word, so the
 *                  following steps are skipped as well and prego_miniroad_check reports PREGO_ETIMEOUT on every rank at the same step. */
/* prego_miniroad_adamw_step for MiniROADA's anticipation_layer.0.{weight, bias} (params[0] [ant_len * hid, hid], params[1] [ant_len * hid];
 * grads / exp_avg / exp_avg_sq likewise), rewriting the handle's anticipation operand copies in the same pass (ABI 7 addition).  Guarded on
 * the device by the same timeout word and peer guard: whenever prego_miniroad_adamw_step changes nothing, neither does this one. */
int prego_miniroad_adamw_step_anticipation(prego_miniroad* h, float* const* params, const float* const* grads, float* const* exp_avg,
                                           float* const* exp_avg_sq, int64_t step, float lr, float beta1, float beta2, float eps,
                                           float weight_decay, prego_stream_t stream);
int prego_miniroad_guard_publish(prego_miniroad* h, float* dst, prego_stream_t stream);
int prego_miniroad_set_peer_guard(prego_miniroad* h, const float* reduced_word);

/* ---- "Transformer" (ViTEnc): step_recognition/model/transformer_models/ViT.py:25-143 ------------------------------ */
typedef struct prego_vit prego_vit;

/* ViTEnc.__init__ (ViT.py:26-90) with patch_dim = 1: emb = cfg['embedding_dim'], mlp = cfg['hidden_dim'] (ViT.py:75),
 * heads = cfg['num_heads'], layers = cfg['num_layers'], window = cfg['window_size'] (the learned positional table pins
 * T == window, PositionalEncoding.py:25-41).  Supported: head dim 64/128/256, emb % 512 == 0, mlp % 128 == 0. */
int prego_vit_create(prego_vit** out, int d_rgb, int d_flow, int emb, int mlp, int heads, int layers, int window,
                     int n_classes);
void prego_vit_destroy(prego_vit* h);
/* number of tensors set_weights expects: 4 + 11 * layers + 4 */
int prego_vit_num_tensors(const prego_vit* h);
/* device fp32 tensors in state_dict order:
 *   linear_encoding.weight [emb, d_in], linear_encoding.bias, cls_token [emb], position_encoding.pe.weight [window+1, emb],
 *   per layer l (a = 2l, f = 2l+1): encoder.net.a.fn.norm.{weight,bias}, encoder.net.a.fn.fn.qkv.weight [3emb, emb],
 *     encoder.net.a.fn.fn.proj.{weight [emb,emb], bias}, encoder.net.f.fn.norm.{weight,bias},
 *     encoder.net.f.fn.fn.net.0.{weight [mlp,emb], bias}, encoder.net.f.fn.fn.net.3.{weight [emb,mlp], bias},
 *   pre_head_ln.{weight,bias}, mlp_head.{weight [n_classes, emb], bias} */
int prego_vit_set_weights(prego_vit* h, const float* const* tensors, int n_tensors, prego_stream_t stream);
size_t prego_vit_workspace_bytes(const prego_vit* h, int batch);
/* MFMA operand type of the handle: PREGO_BF16 (default) or PREGO_F16 (IEEE fp16 operands and 16-bit activations: the same rate
 * and bytes, 8x less operand rounding - logits within 1e-3 of the fp32 reference where bf16 gives 2.5e-3; inference entry points
 * only: forward, forward_frames), or PREGO_F32 (parity mode: the matrices stay fp32, the projections run on the exact-fp32 MFMA
 * GEMM, attention / GELU / residuals in fp32, every block on every token; prego_vit_forward only - logits within 2e-5 of the
 * reference; the north star's "1e-3 fp32" figure is checked on it).  Changing the type invalidates the ingested weights (call
 * set_weights again); prego_vit_workspace_bytes follows the handle's type. */
int prego_vit_set_compute_dtype(prego_vit* h, int compute_dtype);

/* ViTEnc.forward (ViT.py:117-143): rgb/flow device fp32 [batch, window, d_rgb/d_flow] (flow NULL = zeros);
 * out_logits device fp32 [batch, n_classes] (the reference returns it as [batch, 1, n_classes], raw logits in both
 * modes).  flags bit 0: causal self-attention (extension; the reference module has no mask, Attention.py:21-41).
 * The reference reads the encoder output at token 0 only (ViT.py:136), so the LAST block computes its query, attention output,
 * projection and FFN for token 0 of every window only (keys / values for all tokens): exact, 44 % fewer FLOPs at num_layers = 1.
 * flags bit 1 (debug / A-B): run the last block on every token as the reference does. */
int prego_vit_forward(prego_vit* h, int batch, const float* rgb, const float* flow, float* out_logits, int flags,
                      void* workspace, size_t workspace_bytes, prego_stream_t stream);

/* Per-frame inference of the `Transformer` entry over ONE whole video - what trainer/eval.py:36-56 needs from a model whose forward
 * emits one logit vector per window (ViT.py:136-141) and requires T == window_size: out_logits[t] = ViTEnc(window ending at frame
 * t), zero feature rows in front of the video (the training loader's windows, datasets/dataset.py:53-55,96-103, at stride 1).
 * linear_encoding (ViT.py:124) runs once per frame, not once per (window, position); windows go through the encoder
 * `windows_per_batch` at a time.  rgb / flow: device fp32 [n_frames][d_rgb | d_flow] (flow NULL = zeros); out_logits: device fp32
 * [n_frames][n_classes] raw logits (ViTEnc applies no softmax); out_argmax (nullable): device int32 [n_frames], np.argmax of each
 * row (trainer/eval.py:53).  flags bit 0: causal attention.  Workspace: prego_vit_frames_workspace_bytes. */
size_t prego_vit_frames_workspace_bytes(const prego_vit* h, int n_frames, int windows_per_batch);
int prego_vit_forward_frames(prego_vit* h, int n_frames, const float* rgb, const float* flow, float* out_logits, int32_t* out_argmax,
                             int windows_per_batch, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);

/* Transformer stream pool (an addition to ABI 7, existing signatures unchanged): live serving for the `Transformer` entry, the
 * counterpart of prego_stream_pool_* / prego_miniroad_step_pool.  It replaces what a host does around ViTEnc.forward when frames arrive
 * one at a time (trainer/eval.py:36-56 over dataset.py:53-55,96-103 at stride 1, then utils/aggregate.py:46-90 on the argmax): keeping
 * the last window_size feature rows of every stream, rebuilding [n, window_size, d] windows each tick, encoding every frame window_size
 * times (ViT.py:124 does not depend on the position in the window; ViT.py:129 adds the positional row afterwards) and voting on the host.
 * Every live video owns a SLOT of one device block:
 *   ring            fp32 [window_size][embedding_dim]: row f mod window_size = linear_encoding(frame f), bias included - the row
 *                   prego_vit_forward_frames keeps per frame
 *   ring words      int32 head (the next row to write = frames mod window_size), fill (min(frames, window_size)), two spare words
 *   record          the stream pool's vote record, unchanged (prego_stream_pool_* above: layout, update rule, overflow bits)
 *   block           device memory, 256-byte aligned, at least prego_vit_stream_pool_bytes(h, capacity, max_events) bytes, the caller's:
 *                   the rings at offset 0, then the ring words, then the records.  create enqueues its zeroing on `stream`; an all-zero
 *                   slot is an empty stream, so opening a stream needs no call.  window_size * embedding_dim * 4 bytes per slot (512 KB
 *                   at 128 / 1024, 8 MB at 1024 / 2048): the capacity is the caller's choice; _bytes returns 0 and create refuses
 *                   only what size_t cannot hold.  The handle must outlive the pool.
 * prego_vit_step_pool: one new frame for the slots named (HOST int32 [n_active], 1 <= n_active <= min(256, capacity), each inside the
 * pool and named once; free to reuse once the call returns) - the frames are converted and encoded (n_active rows), every row goes into
 * its slot's ring, one window per slot is read out of the rings (token j: cls + pe[T] for j == T; the bias row + pe[j] where the stream
 * has fewer than T - j frames, a zero feature row in front of the video; else ring[(head + j) mod T] + pe[j]), the encoder blocks and the
 * head run exactly as prego_vit_forward_frames runs them for a batch of n_active windows, and every slot's record takes its argmax.
 * rgb / flow: device fp32 [n_active][d_rgb | d_flow] (flow NULL = zeros), row i belongs to slots[i]; out_logits: device fp32
 * [n_active][n_classes] raw logits; argmax (nullable: the ids go through the workspace): device int32 [n_active].  flags bit 0: causal
 * attention.  Bits: the same streams pushed in the same order with the same n_active give the same bits whatever their slot numbers; the
 * GEMM kernels are chosen by row count, so logits are NOT promised bit-identical to prego_vit_forward_frames or to a call with another
 * n_active (they agree to the tolerance that holds prego_vit_forward_frames against prego_vit_forward).  No device allocation, no host wait.
 *   workspace       device memory, 256-byte aligned, prego_vit_step_pool_workspace_bytes(h, n_active) bytes
 * prego_vit_stream_pool_flush / _reset / _record: prego_stream_pool_flush / _reset / _record for this pool; reset zeroes head, fill and
 * the record and leaves the ring rows (nothing reads a row that fill does not cover).  prego_vit_stream_pool_window: the slot's logical
 * window, oldest frame first, into out (device fp32 [window_size][embedding_dim]; bias rows where fill does not reach) and fill into
 * fill_out (device int32, nullable): for inspection.
 * PREGO_EINVAL / PREGO_EWORKSPACE with a message, nothing launched: an fp32-operand handle, a call before set_weights, n_active outside
 * 1..min(256, capacity), a slot outside the pool, a slot named twice, a NULL, unaligned or too small block or workspace, vote_window < 1,
 * max_events outside 1..1 048 576, a pool created for another window_size, embedding_dim or class count, a missing input.  Not covered:
 * a dense step without a pool, the fp32 parity mode.  A pool belongs to one stream at a time.
 * prego_vit_step_pool_bursts: counts[i] new frames (HOST int32 [n_active], 1 <= counts[i] <= min(32, window_size)) for slots[i] in one
 * call, R = sum(counts) <= 256 packed rows in `slots` order: slot i owns rows off[i] .. off[i] + counts[i]), off the prefix sums.  One
 * window per packed row comes back - the window ending at that frame.  With head / fill the slot's ring words before the call and
 * d = T - 1 - j, token j < T of the window of (slot i, burst frame k) is: the call's own encoded row off[i] + k - d where d <= k; the bias
 * row where d - k > fill; else ring[(head - (d - k)) mod T] as it was before the call; each + pe[j].  Afterwards the slot's ring, head
 * and fill are byte for byte what counts[i] calls of prego_vit_step_pool with the same rows leave, and its record has taken the
 * counts[i] ids in frame order (a vote-window boundary may fall inside a burst).  rgb / flow: device fp32 [R][d_rgb | d_flow]; out_logits
 * [R][n_classes]; argmax (nullable) int32 [R].  The encoding GEMM runs once at M = R and the blocks once for R windows; the GEMM kernels
 * are chosen by row count, so a burst's logits agree with R one-frame calls to the tolerance above, not bit for bit (every count 1:
 * the same shapes, the same bits).  Refused as prego_vit_step_pool refuses, and: counts NULL, a count outside 1..min(32, window_size),
 * R > 256.  Workspace: prego_vit_step_pool_bursts_workspace_bytes(h, n_active, R) bytes (0 for a shape the call refuses). */
typedef struct prego_vit_stream_pool prego_vit_stream_pool;
size_t prego_vit_stream_pool_bytes(const prego_vit* h, int capacity, int max_events);
int prego_vit_stream_pool_create(prego_vit_stream_pool** out, const prego_vit* h, int capacity, int vote_window, int max_events,
                                 void* device_block, size_t bytes, prego_stream_t stream);
void prego_vit_stream_pool_destroy(prego_vit_stream_pool* p);
size_t prego_vit_step_pool_workspace_bytes(const prego_vit* h, int n_active);
int prego_vit_step_pool(prego_vit* h, prego_vit_stream_pool* p, int n_active, const int32_t* slots, const float* rgb, const float* flow,
                        float* out_logits, int32_t* argmax, int flags, void* workspace, size_t workspace_bytes, prego_stream_t stream);
size_t prego_vit_step_pool_bursts_workspace_bytes(const prego_vit* h, int n_active, int n_rows);
int prego_vit_step_pool_bursts(prego_vit* h, prego_vit_stream_pool* p, int n_active, const int32_t* counts, const int32_t* slots,
                               const float* rgb, const float* flow, float* out_logits, int32_t* argmax, int flags, void* workspace,
                               size_t workspace_bytes, prego_stream_t stream);
int prego_vit_stream_pool_flush(prego_vit_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream);
int prego_vit_stream_pool_reset(prego_vit_stream_pool* p, int n, const int32_t* slots, prego_stream_t stream);
int prego_vit_stream_pool_record(const prego_vit_stream_pool* p, int slot, const void** device_record, size_t* bytes);
int prego_vit_stream_pool_window(prego_vit_stream_pool* p, int slot, float* out, int32_t* fill_out, prego_stream_t stream);

/* Event feed of a stream pool (an addition to ABI 7, existing signatures unchanged): what changed in ANY slot since the previous drain, in
 * one small report - for a live consumer that acts when a new step appears (step_anticipation), without one record copy per slot per
 * tick.  One feed serves either pool type; it reads the pool's records and never writes the pool's block.
 *   feed block      device memory, 256-byte aligned, at least prego_stream_pool_feed_bytes(capacity, max_out) bytes, the caller's; create
 *                   enqueues its zeroing on `stream`.  One cursor word per slot - bits 0..29 the slot's events already delivered, bits
 *                   30..31 the overflow bits (record full, id out of range) already reported -, the drain counter and one word of
 *                   scratch per 256 slots.
 *   report          device memory, 256-byte aligned, at least prego_stream_pool_feed_report_bytes(max_out) bytes, the caller's and
 *                   separate from the feed block, so several may be in flight.  int32 words: count | pending | seq | 0, then max_out
 *                   entries slot | index | step id | first frame (16 bytes each); `index` is the event's position in the slot's record.
 *                   An entry with index -1 reports a slot's newly set overflow bits, once: the bits in the id field, the slot's
 *                   `frames` in the last.
 * prego_stream_pool_feed_drain: for every slot of the pool, n_events (clamped to 0..max_events) and the overflow word are read; when
 * n_events is below the cursor's count, or a bit the cursor holds as reported is no longer set, the record was reset behind the feed's
 * back and the cursor restarts at 0; the entries due are the slot's newly set overflow bits (if any), then its events
 * [delivered, n_events).  Entries are written in ascending slot order, then ascending index (-1 first) - a function of the slot numbers
 * alone, whatever the capacity.  When more than max_out entries are due the first max_out in that order are written, the cursors move
 * only past what was written (a slot may be delivered in part), `pending` holds the count left behind (saturating at 2^31 - 1) and the
 * next drain goes on from there: nothing is lost, nothing is delivered twice.  The header is always written (count 0 when nothing is
 * new); nothing is written behind entry `count`; seq counts the drains of this feed from 1.  Two launches (one for a pool of up to 256
 * slots); no atomics, no workgroup waits for another, no device allocation, no host wait.
 * prego_stream_pool_feed_forget: zeroes the cursors of the slots named (HOST int32 [n], the pool calls' rules), for a slot that was
 * reset and handed to a new stream.
 * PREGO_EINVAL / PREGO_EWORKSPACE (a block or report too small) with a message, nothing launched: a NULL feed, pool, block, report or
 * slot list, an unaligned block or report, max_out outside 1..16 777 216, n outside 1..min(256, capacity), a slot outside the pool or
 * named twice.  The pool's block must outlive the feed; a feed belongs to the stream its pool belongs to. */
typedef struct prego_stream_pool_feed prego_stream_pool_feed;
size_t prego_stream_pool_feed_bytes(int capacity, int max_out);
size_t prego_stream_pool_feed_report_bytes(int max_out);
int prego_stream_pool_feed_create(prego_stream_pool_feed** out, const prego_stream_pool* p, int max_out, void* device_block, size_t bytes,
                                  prego_stream_t stream);
int prego_vit_stream_pool_feed_create(prego_stream_pool_feed** out, const prego_vit_stream_pool* p, int max_out, void* device_block,
                                      size_t bytes, prego_stream_t stream);
void prego_stream_pool_feed_destroy(prego_stream_pool_feed* f);
int prego_stream_pool_feed_drain(prego_stream_pool_feed* f, void* report, size_t report_bytes, prego_stream_t stream);
int prego_stream_pool_feed_forget(prego_stream_pool_feed* f, int n, const int32_t* slots, prego_stream_t stream);

/* Slot images of a stream pool (an addition to ABI 7, existing signatures unchanged): a live slot taken out of a pool as data and put
 * into a pool again - another pool, other slot numbers, another device or another process by way of the host -, bit for bit the stream
 * it was, with its feed position.  Both pool types.  An image is only meaningful for the weights that made it: the geometry is checked,
 * the weights are the caller's business.
 * Image of a slot: prego_stream_pool_image_bytes(p) bytes (a multiple of 256), the same for every slot of a pool, 32-bit words:
 *   tag    [16]  magic 0x474d4950 | image version 1 | kind (1 GRU pool, 2 Transformer pool) | hid or embedding_dim | window_size (0 for
 *                the GRU pool) | n_classes | vote window | max_events | frames | ring head | ring fill | feed cursor word (0 when no feed
 *                was named) | 0 | 0 | 0 | 0
 *   state        GRU pool: the fp32 state row [hid].  Transformer pool: the ring [window_size][embedding_dim] fp32 at its physical row
 *                positions, the rows that fill does not cover (fill .. window_size - 1) as zeros
 *   record       the slot's vote record, all of its words: frames | last vote + 1 | n_events | overflow | counts[n_classes rounded up
 *                to 4] | event_id[max_events] | event_start[max_events]
 *   zeros        up to the next multiple of 256 bytes
 * An image is canonical: the same stream gives the same bytes whatever slot it lived in and whatever lived there before.
 * prego_stream_pool_snapshot: images[i] <- slot slots[i]; the pool's block is only read.  With a feed, the slot's cursor word travels
 * in the tag.  One launch.
 * prego_stream_pool_restore: slot slots[i] <- images[i]: state or ring, ring words, record and, with a feed, its cursor word for the
 * slot.  Every image is validated on the device before anything of its slot is written; an image that fails leaves its slot and the
 * feed's cursor byte for byte as they were.  status (device int32 [n], nullable): 0 = restored, else a bit per failed clause -
 *   1   tag words 0..7 differ from the pool's geometry       2   frames < 0, or the record's frames is not the tag's
 *   4   n_events outside 0..max_events                        8   last vote + 1 outside 0..n_classes
 *   16  overflow word outside 0..3                            32  a counter outside 0..vote window
 *   64  Transformer pool: head != frames mod window_size or fill != min(frames, window_size)
 *   128 the cursor's delivered count (bits 0..29) is above n_events
 * One launch; no atomics, no workgroup waits for another.  The caller reads status when it wants to know; restoring into a slot that
 * holds a stream overwrites it.
 * slots: HOST int32 [n], n in 1..min(256, capacity), inside the pool, each named once.  images: device memory, 256-byte aligned, at
 * least n * image_bytes, outside the pool's and the feed's blocks.  PREGO_EINVAL / PREGO_EWORKSPACE (images too small) with a message,
 * nothing launched: a NULL pool, slot list or images, a feed that belongs to another pool, unaligned or overlapping memory.  No device
 * allocation, no host wait. */
size_t prego_stream_pool_image_bytes(const prego_stream_pool* p);
int prego_stream_pool_snapshot(prego_stream_pool* p, const prego_stream_pool_feed* feed /* nullable */, int n, const int32_t* slots,
                               void* images, size_t bytes, prego_stream_t stream);
int prego_stream_pool_restore(prego_stream_pool* p, prego_stream_pool_feed* feed /* nullable */, int n, const int32_t* slots,
                              const void* images, size_t bytes, int32_t* status /* nullable */, prego_stream_t stream);
size_t prego_vit_stream_pool_image_bytes(const prego_vit_stream_pool* p);
int prego_vit_stream_pool_snapshot(prego_vit_stream_pool* p, const prego_stream_pool_feed* feed /* nullable */, int n, const int32_t* slots,
                                   void* images, size_t bytes, prego_stream_t stream);
int prego_vit_stream_pool_restore(prego_vit_stream_pool* p, prego_stream_pool_feed* feed /* nullable */, int n, const int32_t* slots,
                                  const void* images, size_t bytes, int32_t* status /* nullable */, prego_stream_t stream);

/* Procedure model (an addition to ABI 7, existing signatures unchanged): online mistake detection from a corpus of correct step
 * transcripts - the symbolic, integer-exact stand-in for step_anticipation's LLM branch.  Definitions:
 *   symbols   step ids 0 .. n_classes - 1 (1 <= n_classes <= 128); a virtual START stands in front of every sequence.
 *   corpus    transcripts, each with a group id >= 0 (the toy class), its symbols and a target flag per position.  A target position p
 *             is an EXAMPLE: context START, s_0 .. s_{p-1}, next symbol s_p.
 *   query     a history START, e_0 .. e_{i-1}, the current step e_i and a group q; q = -1: every group.  A queried symbol outside
 *             [0, n_classes) equals nothing.  A group without examples (or outside the corpus's groups) has none.
 *   match     for 1 <= j <= order (1..8) an example matches at j when both contexts hold at least j symbols, START included, and their
 *             last j symbols are equal.  tot_j: the matching examples of the group; cnt_j(c): those whose next symbol is c.
 *   j*        the largest j <= min(order, i + 1) with tot_j > 0; none: the verdict is UNKNOWN (not a mistake).
 *   allowed   class c, when cnt(c) > 0 and cnt(c) * den >= tot * num at j* (64-bit products; 0 <= num <= den <= 32768).  MISTAKE: e_i
 *             is not allowed.  order 1 with num/den = 1/N is the rule of step_anticipation/src/data/frequentist_baseline.py.
 *   verdict   8 int32 words (two 16-byte stores): flags | cnt(e_i) | tot | group used | allowed mask, bits 0..31 | 32..63 | 64..95 |
 *             96..127.  flags: 1 JUDGED, 2 MISTAKE, 4 UNKNOWN, 8 SKIPPED, j* in bits 8..15.  A SKIPPED verdict is 8 | 0 | 0 | -1 | 0 ...
 * prego_procedure_model_create: validates the corpus on the host - transcripts t = 0 .. n_transcripts - 1 (HOST arrays) with group
 * groups[t] in 0..2^20 - 1, symbols[offsets[t] .. offsets[t + 1]) each in [0, n_classes), targets (nullable: every position) one byte per
 * symbol -, sorts it by group and enqueues ONE copy of the laid-out corpus into device_block: device memory, 256-byte aligned, at least
 * prego_procedure_model_bytes(n_groups = 1 + the largest group, n_transcripts, n_symbols, n_examples) bytes, the caller's, only read
 * afterwards.  Caps, from the word widths: n_symbols + n_transcripts <= 2^30 (a position is an int32 word), n_examples <= 2^24 (counts
 * are int32 words; cnt * den fits 64 bits), 2^20 groups.  The model object holds host memory only; the block must outlive it.
 * prego_procedure_judge (the offline / evaluation entry): sequence s = symbols[offsets[s] .. offsets[s + 1]) with group groups[s], all
 * DEVICE int32 (offsets [n_sequences + 1] ascending from 0 to n_positions); verdict t judges symbols[t] after its sequence's symbols in
 * front of it.  verdicts: device, 256-byte aligned, n_positions * 32 bytes.
 * prego_stream_pool_feed_judge / prego_vit_stream_pool_feed_judge: `report` is what prego_stream_pool_feed_drain wrote earlier on the
 * same stream, still on the device; its count is read there.  Verdict k judges entry k: e_i = the entry's step id, the history the
 * slot's record event_id[.. index - 1], the group slot_groups[slot] (DEVICE int32 [capacity], the caller's).  An overflow entry
 * (index -1), a slot outside the pool or an index at or beyond the record's n_events (clamped to 0..max_events) is SKIPPED.  verdicts:
 * device, 256-byte aligned, max_out * 32 bytes; nothing is written behind verdict `count`.  The pool's block, the report and the model
 * are only read.
 * One launch each, one wave per judged item over a bounded grid; integers only, no global atomics (a verdict is a function of the
 * inputs alone), no device allocation, no host wait.  PREGO_EINVAL / PREGO_EWORKSPACE (a block or buffer too small) with a message,
 * nothing copied or launched: a NULL argument, an unaligned block, report or verdict buffer, n_classes, order, threshold, a group or a
 * symbol out of range, descending offsets, a corpus beyond the caps. */
typedef struct prego_procedure_model prego_procedure_model;
size_t prego_procedure_model_bytes(int n_groups, int64_t n_transcripts, int64_t n_symbols, int64_t n_examples);
int prego_procedure_model_create(prego_procedure_model** out, int n_classes, int order, int thr_num, int thr_den, int n_transcripts,
                                 const int32_t* groups, const int64_t* offsets, const int32_t* symbols, const uint8_t* targets /* nullable */,
                                 void* device_block, size_t bytes, prego_stream_t stream);
void prego_procedure_model_destroy(prego_procedure_model* m);
int prego_procedure_judge(const prego_procedure_model* m, int n_sequences, int n_positions, const int32_t* offsets, const int32_t* symbols,
                          const int32_t* groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream);
int prego_stream_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                 const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream);
int prego_vit_stream_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                     const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream);

/* Next-step forecast from the procedure model (an addition to ABI 7, existing signatures unchanged): the histogram a verdict is read
 * from, handed out ranked.  Definitions (everything of 13l above holds):
 *   query     a history START, e_0 .. e_{n-1} with n >= 0 steps, all of them context, and a group q.  len = min(order, n + 1).
 *   j*        the largest j <= len with tot_j > 0; none: the forecast is UNKNOWN.
 *   ranked    the candidates - classes with cnt_{j*}(c) > 0 - by count descending, equal counts by ascending class id; the forecast
 *             holds the first min(8, n_cand).  The allowed mask is the verdict's rule on the same row.
 *   identity  the forecast after e_0 .. e_{i-1} in group q has the j*, tot and allowed mask of the verdict of e_i after that history.
 *   forecast  24 int32 words (six 16-byte stores): flags | n_cand | tot | group used | allowed mask [4] | id [8] | cnt [8].  flags: 1 MADE,
 *             4 UNKNOWN, 8 SKIPPED, j* in bits 8..15, ranked entries (0..8) in bits 16..19; unused ranks hold id -1, cnt 0.
 *             UNKNOWN: 1|4, 0, 0, group, 0 x 4, -1 x 8, 0 x 8.  SKIPPED: 8, 0, 0, -1, 0 x 4, -1 x 8, 0 x 8.
 * prego_procedure_forecast (offline): the sequences as prego_procedure_judge takes them, except that n_positions may be 0 (every
 * sequence empty; symbols still not NULL).  Sequence s with L_s symbols yields L_s + 1 forecasts, after its first p = 0 .. L_s symbols,
 * at row offsets[s] + s + p: n_positions + n_sequences rows.  Row (s, p) forecasts symbol p; the last row what would follow the sequence.
 * prego_stream_pool_feed_forecast / prego_vit_stream_pool_feed_forecast: the arguments of _feed_judge.  Forecast k says what comes
 * after entry k: its history is the slot's event_id[.. index - 1] followed by the entry's own step id.  SKIPPED as _feed_judge; nothing
 * is written behind forecast `count`.
 * prego_stream_pool_forecast / prego_vit_stream_pool_forecast: slots (DEVICE int32 [n], 1 <= n <= capacity; a slot may repeat) and
 * slot_groups (DEVICE int32 [capacity]).  Forecast i says what comes after every event slot slots[i]'s record holds (n_events clamped to
 * 0..max_events; none: a START-only query); a slot outside the pool is SKIPPED.
 * forecasts: device, 16-byte aligned, 96 bytes per row.  One launch each, a wave per row; integers only, no global atomics, no device
 * allocation, no host wait.  PREGO_EINVAL / PREGO_EWORKSPACE (a buffer too small) with a message, nothing launched: a NULL argument, an
 * unaligned buffer, n or the sequence counts out of range. */
int prego_procedure_forecast(const prego_procedure_model* m, int n_sequences, int n_positions, const int32_t* offsets, const int32_t* symbols,
                             const int32_t* groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);
int prego_stream_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                    const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);
int prego_vit_stream_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report,
                                        size_t report_bytes, const int32_t* slot_groups, void* forecasts, size_t forecast_bytes,
                                        prego_stream_t stream);
int prego_stream_pool_forecast(const prego_stream_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                               const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);
int prego_vit_stream_pool_forecast(const prego_vit_stream_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                                   const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);

/* Decode pool (an addition to ABI 7, existing signatures unchanged): online fixed-lag Viterbi per live stream on the device - the
 * decoder of prego_viterbi_decode for streams whose last frame has not arrived.  Every live stream owns a SLOT of one device block that
 * holds its Viterbi state; a push of score rows advances any subset of the slots; every frame's label is committed a fixed number of
 * frames (`lag`) after it arrived, and the committed labels feed a vote record of the stream pools' layout, so the event feed and both
 * monitors work on the decoded transcript unchanged.
 * DEFINITIONS.  The model and the quantiser are prego_viterbi_decode's.
 *   - trans[i][j] and init[j] are int32.
 *   - A negative word is forbidden.  A word above PREGO_DECODE_CAP is read as CAP.  init NULL means zeros.
 *   - At most 128 classes.
 *   - Emission costs come from the fp32 word by DECODE_LUT, or from int32 cost words clamped into [0, CAP].
 *   - d_0, d_t and the back-pointer (lowest i on a tie) are as in viterbi_decode.
 *   - e_t is the lowest j with the smallest finite d_t(j).
 * FIXED LAG L (0..256).
 *   - After frame t of a stream has been ingested and t >= L, frame f = t - L is committed.  label(f) is the state at frame f on the
 *     back-pointer chain that starts at e_t.
 *   - flush commits the remaining frames [max(0, T - L), T) from the chain that starts at e_{T-1}.
 *   - Dead streams: a frame at which no state is finite makes the stream dead.  Every label committed from then on is -1, at flush too.
 *     Labels already committed stay.
 * Equivalently, and this is the oracle identity:  label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f].
 * After T frames, (cost, end state) equals viterbi_decode(x[:T])'s record.  With L >= T - 1 the labels equal the offline decode.
 * Consecutive labels come from different chains, so the committed sequence need not be an allowed path.
 * The result depends on the frames only.  It does not depend on how they were cut into calls, on slot numbers, on the order of `slots`,
 * or on the other slots.
 * RECORD.  Each committed label goes, in frame order, through the stream pools' update rule into a record of their layout (window =
 * vote_window; with 1 every change of the committed label is an event: id, first frame).  A label of -1 sets the bad-id bit and counts
 * no frame, as an id outside the classes does there.
 * BLOCK.  Device memory, 256-byte aligned, at least prego_decode_pool_bytes(capacity, n_classes, lag, max_events) bytes, the caller's:
 * the clamped model, then per slot a header, the keys d as int64 [n_classes rounded up to 4] (d << 7 | state; "no path" 2^62; exact,
 * finite d < 2^47, nothing saturates) and a ring of back-pointer rows, one byte per (frame, state), addressed by frame index modulo
 * lag + 32; then the records.  create enqueues the block's zeroing and one small kernel that clamps trans / init (DEVICE int32
 * [n_classes][n_classes] / [n_classes] or NULL) into it on `stream`; the caller may free them stream-ordered.  An all-zero slot is an
 * empty stream, so opening a slot needs no call.
 * prego_decode_pool_push / _push_costs (int32 cost rows): slots HOST int32 [n] (the stream pools' rules: 1 <= n <= min(256, capacity),
 * inside the pool, named once); counts HOST int32 [n], 1..32 each, with sum R <= 256; rows DEVICE [R][ld] packed in `slots` order,
 * ld >= n_classes (4-byte aligned is enough; words behind n_classes are not read).  Outputs are device pointers and all nullable:
 *   labels   int32 [R].  In slot i's row block, the first m_i words are the labels this call committed in frame order.  The rest are
 *            PREGO_DECODE_PENDING.
 *   commit   int32 [n][2]: (index of the first frame committed by this call, or of the next one due when m_i = 0; m_i).
 *   now      int32 [R]: e_t of every ingested frame, -1 once dead.  This is the zero-lag provisional label.
 * One launch, one 256-thread workgroup per named slot (csrc/decode_pool.hip); no workspace, no global atomic, no float arithmetic, no
 * allocation, no host wait.
 * prego_decode_pool_flush: commits the tail (labels DEVICE int32 [n][lag], nullable: slot i's labels then PREGO_DECODE_PENDING; commit
 * as above), then votes the record's unfinished window as prego_stream_pool_flush does, and marks the slot flushed.  A push on a
 * flushed slot ingests nothing, writes PREGO_DECODE_PENDING into its rows of labels and now, (next frame, 0) into commit, and sets
 * status bit 2.  Only reset reopens it.  prego_decode_pool_reset zeroes the slots; prego_decode_pool_record as for the other pools.
 * prego_decode_pool_state: the slot's header and keys for one D2H copy.  int32 words frames | committed | status (bit 0 dead, bit 1
 * flushed, bit 2 pushed after flush) | end state (-1 dead; 0 while empty) | total cost as int64 (-1 dead) | two zero words, then the keys.
 * prego_decode_pool_feed_create / _feed_judge / _feed_forecast / prego_decode_pool_forecast: the prego_stream_pool_ entries of those
 * names over this pool's records.
 * PREGO_EINVAL with a message, decided before any launch (pool and outputs untouched): everything the slot lists of the other pools
 * refuse; a count outside 1..32, or R > 256; n_classes outside 1..128; lag outside 0..256; vote_window < 1; capacity or max_events
 * outside 1..1 048 576; ld < n_classes; NULL rows, counts or trans; a NULL, unaligned or short block; a procedure model of another
 * class count; outputs overlapping the rows, the block or each other; trans or init inside the block. */
#define PREGO_DECODE_POOL_MAX_LAG 256
#define PREGO_DECODE_PENDING (-2)
typedef struct prego_decode_pool prego_decode_pool;
size_t prego_decode_pool_bytes(int capacity, int n_classes, int lag, int max_events);
int prego_decode_pool_create(prego_decode_pool** out, int capacity, int n_classes, int lag, int vote_window, int max_events,
                             const int32_t* trans, const int32_t* init /* nullable */, void* device_block, size_t bytes,
                             prego_stream_t stream);
void prego_decode_pool_destroy(prego_decode_pool* p);
int prego_decode_pool_push(prego_decode_pool* p, int n, const int32_t* slots, const int32_t* counts, const float* probs, int64_t ld,
                           int32_t* labels, int32_t* commit, int32_t* now, prego_stream_t stream);
int prego_decode_pool_push_costs(prego_decode_pool* p, int n, const int32_t* slots, const int32_t* counts, const int32_t* costs, int64_t ld,
                                 int32_t* labels, int32_t* commit, int32_t* now, prego_stream_t stream);
int prego_decode_pool_flush(prego_decode_pool* p, int n, const int32_t* slots, int32_t* labels, int32_t* commit, prego_stream_t stream);
int prego_decode_pool_reset(prego_decode_pool* p, int n, const int32_t* slots, prego_stream_t stream);
int prego_decode_pool_record(const prego_decode_pool* p, int slot, const void** device_record, size_t* bytes);
int prego_decode_pool_state(const prego_decode_pool* p, int slot, const void** device_state, size_t* bytes);
int prego_decode_pool_feed_create(prego_stream_pool_feed** out, const prego_decode_pool* p, int max_out, void* device_block, size_t bytes,
                                  prego_stream_t stream);
int prego_decode_pool_feed_judge(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                 const int32_t* slot_groups, void* verdicts, size_t verdict_bytes, prego_stream_t stream);
int prego_decode_pool_feed_forecast(const prego_stream_pool_feed* f, const prego_procedure_model* m, const void* report, size_t report_bytes,
                                    const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);
int prego_decode_pool_forecast(const prego_decode_pool* p, const prego_procedure_model* m, const int32_t* slots, int n,
                               const int32_t* slot_groups, void* forecasts, size_t forecast_bytes, prego_stream_t stream);

/* Training of the "Transformer" registry entry: trainer/train.py:20-24 (fwd, loss, backward) over ViTEnc (ViT.py:117-143,
 * Transformer.py:5-82, Attention.py:21-41).  forward_train is ViTEnc.forward in training mode with every dropout rate 0
 * (cfg['dropout'] == cfg['attn_dropout_rate'] == 0; non-zero rates are rejected by the host module) and keeps the activations
 * the backward needs in `workspace` (caller-owned, prego_vit_train_workspace_bytes, untouched between the two calls).
 * backward: dlogits device fp32 [batch, n_classes] = dLoss/dlogits (OadLoss: prego_oad_loss on the [batch,1,C] logits);
 * grads: host array of n_tensors device fp32 tensors in prego_vit_set_weights' order and shapes, OVERWRITTEN.  All sums over
 * rows / windows run in a fixed order (bit-reproducible); the attention backward recomputes the probabilities from Q, K and the
 * forward's log-sum-exp (no [B,h,N,N] tensor) and uses no atomics.  flags bit 0: causal attention (as in forward). */
/* The nn.Dropout layers of the training-mode forward.  p = cfg['dropout']: pe_dropout (ViT.py:130), PreNormDrop after the
 * attention block (Transformer.py:24-32) and the two Dropouts of FeedForward (Transformer.py:41,46).  attn_p =
 * cfg['attn_dropout_rate']: the attention probabilities inside the attention kernel (Attention.py:17,36) and proj_drop
 * (Attention.py:19,40).  All are stateless hash masks of (seed, site, element), regenerated by backward. */
int prego_vit_set_dropout(prego_vit* h, float p, float attn_p, uint64_t seed);
size_t prego_vit_train_workspace_bytes(const prego_vit* h, int batch);
int prego_vit_forward_train(prego_vit* h, int batch, const float* rgb, const float* flow, float* out_logits, int flags,
                            void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_vit_backward(prego_vit* h, int batch, const float* dlogits, float* const* grads, int n_tensors, int flags,
                       void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* optimizer.step() (train.py:24, AdamW of main.py:62-67) for the handle's tensors (prego_vit_set_weights' order and shapes):
 * prego_adamw_step's arithmetic, and the handle's converted copies (bf16 matrices, fp32 vectors) are rewritten from the updated
 * values in the same pass - no prego_vit_set_weights (5 + 4 per layer conversions and 10 + 7 per layer copies) after the step. */
int prego_vit_adamw_step(prego_vit* h, float* const* params, const float* const* grads, float* const* exp_avg,
                         float* const* exp_avg_sq, int n_tensors, int64_t step, float lr, float beta1, float beta2, float eps,
                         float weight_decay, prego_stream_t stream);

/* AttentionLayer(FullAttention(mask_flag=causal)) of attn.py:139-170,35-57,10-18 as a stateless op (BASELINE config 4:
 * long-window causal attention).  x, out: device fp32 [batch, len, d_model]; projection weights [d_model, d_model] and
 * biases [d_model] in nn.Linear layout.  scores = softmax(mask(q k^T) / sqrt(d_model/heads)); never materialised. */
size_t prego_attention_layer_workspace_bytes(int batch, int len, int d_model);
int prego_attention_layer_forward(int batch, int len, int d_model, int heads, int causal, const float* x, const float* wq,
                                  const float* bq, const float* wk, const float* bk, const float* wv, const float* bv,
                                  const float* wo, const float* bo, float* out, void* workspace, size_t workspace_bytes,
                                  prego_stream_t stream);

/* The same layer as a handle: the projection weights are converted once by set_weights (nn.Linear layout, as above), forward
 * then only moves activations.  x, out: device fp32 [batch, len, d_model]. */
typedef struct prego_attn_layer prego_attn_layer;
int prego_attention_layer_create(prego_attn_layer** out, int d_model, int heads);
void prego_attention_layer_destroy(prego_attn_layer* h);
/* PREGO_BF16 (default), PREGO_F16 or PREGO_F32 (parity mode: fp32 projections and fp32 attention, handle_forward only) operands
 * for the handle's forward; changing the type invalidates the ingested weights; handle_workspace_bytes follows the type. */
int prego_attention_layer_set_compute_dtype(prego_attn_layer* h, int compute_dtype);
int prego_attention_layer_set_weights(prego_attn_layer* h, const float* wq, const float* bq, const float* wk, const float* bk,
                                      const float* wv, const float* bv, const float* wo, const float* bo, prego_stream_t stream);
size_t prego_attention_layer_handle_workspace_bytes(const prego_attn_layer* h, int batch, int len);
int prego_attention_layer_handle_forward(prego_attn_layer* h, int batch, int len, int causal, const float* x, float* out,
                                         void* workspace, size_t workspace_bytes, prego_stream_t stream);
/* The layer under autograd (attn.py:151-170 inside loss.backward(), trainer/train.py:20-24): forward_train is handle_forward that
 * keeps x, q, k, v, the attention output (bf16) and the row log-sum-exp in `workspace`; backward reads them from the SAME
 * workspace and overwrites grads[0..7] (fp32, set_weights order: wq, bq, wk, bk, wv, bv, wo, bo) and, if not NULL,
 * dx [batch, len, d_model] (queries = keys = values = x: the three input gradients summed).  bf16 handles only; the
 * attention_dropout of attn.py:39,54 (nn.Dropout on A = softmax(scale * scores), active under module.train()): prego_attention_layer_set_dropout
 * below, p = 0 by default (the state the reference's modules are in under .eval()). */
/* FullAttention(attention_dropout = p) in training mode: every forward_train / backward pair that follows drops each attention probability
 * with probability p and scales the survivors by 1 / (1 - p) (the softmax denominator sums the undropped row), by a stateless hash of
 * (seed, element) - pass a fresh seed per step; the backward regenerates the mask of its forward.  0 <= p < 1. */
int prego_attention_layer_set_dropout(prego_attn_layer* h, float p, uint64_t seed);
size_t prego_attention_layer_train_workspace_bytes(const prego_attn_layer* h, int batch, int len);
int prego_attention_layer_forward_train(prego_attn_layer* h, int batch, int len, int causal, const float* x, float* out,
                                        void* workspace, size_t workspace_bytes, prego_stream_t stream);
int prego_attention_layer_backward(prego_attn_layer* h, int batch, int len, int causal, const float* dout, float* dx,
                                   float* const* grads, int n_tensors, void* workspace, size_t workspace_bytes,
                                   prego_stream_t stream);

/* Environment switches THIS library reads (each once, when a handle is created; none is needed in production).  Four, each between two
 * code paths that the driver-run GPU tests hold bit-identical to each other:
 *   PREGO_SPLIT_PASS      0 = never the split pass, R = on R XCDs whenever a call is eligible; unset = per call (cost model)   tests/test_gpu_split.py
 *   PREGO_NO_XCD_OVERLAP  no layer1 worker on the XCDs a thinned-out recurrence has left (the serial chunked pass)            tests/test_gpu_fullsize.py
 *   PREGO_GRU_NO_LOCAL    never the XCD-local hand-off of the recurrence (sc1 stores / loads everywhere)                      tests/test_gpu_miniroad.py
 *   PREGO_GRU_NO_MT       multi-tile steps on the classic recurrence kernel                                                   tests/test_gpu_fullsize.py
 * Every tuning / calibration / diagnostic knob (PREGO_SPLIT_LAG1..3, PREGO_SPLIT_CHUNK_SHIFT, PREGO_SPLIT_GI_RING, PREGO_SPLIT_STATS, PREGO_PLAN_SLOTS,
 * PREGO_SIDE_PRIO, PREGO_PACK_*, PREGO_GRU_STAMPS, PREGO_GRU_MT_SPEC, PREGO_GEMM_NO_*, PREGO_HEAD_V1, PREGO_ATTN_NW, ...) is read by
 * libprego_amd_debug.so ONLY (csrc/kernels.h: prego_tune_env returns NULL in this library), like the probe / unit-test entry points
 * (prego_debug_*, prego_miniroad_debug_stamps: include/prego_amd_debug.h; the same sources built with -DPREGO_DEBUG_ABI). */

#ifdef __cplusplus
}
#endif
#endif /* PREGO_AMD_H */
