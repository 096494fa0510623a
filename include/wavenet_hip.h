/* wavenet_hip.h -- C ABI of libwavenet_hip.so (MI355X / gfx950 WaveNet-vocoder training path).
 *
 * Drop-in boundary.  The reference (kan-bayashi/PytorchWaveNetVocoder) has no FFI: its boundary
 * is the Python API of wavenet_vocoder.nets.  This library is what a binding of
 * that API calls instead of torch.nn ops; every entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain C types only: device pointers + sizes; the caller (PyTorch-ROCm, or any HIP program)
 *     owns every buffer, the library allocates no device memory and keeps no state between calls
 *     (one exception: the opt-in overlap modes WN_FLAG_BWD_OVERLAP / WN_FLAG_FWD_OVERLAP create ONE internal
 *     non-blocking stream and a few events per device on first use);
 *   - activations are channel-major fp32 (B, C, T) exactly like the reference's tensors; sample
 *     indices are int64 (torch.long); logits are written physically as (B, Q, T) -- the
 *     reference's `(B, T, Q)` result is the `.transpose(1, 2)` view of that buffer
 *     (wavenet.py:522 does the same);
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream); no hidden synchronisation; re-entrant per stream;
 *   - return value 0 = ok; non-zero = error, text via wn_last_error() (thread local).
 *
 * Parameters live in ONE flat fp32 buffer (and gradients / Adam moments in buffers of the same
 * shape).  The flat order is the order in which the backward pass finishes gradients
 *      [conv_post_2, conv_post_1, skip_1x1.0..L-1] [layer L-1] ... [layer 0] [causal, upsampling]
 * so that data-parallel gradient buckets are contiguous ranges that become ready front to back.
 * Inside the buffer every tensor keeps the reference's own layout (Conv1d weight (Cout,Cin,K)
 * etc.), so nn.Parameter views of it carry the reference's state_dict keys and shapes
 * (wavenet.py:187-210).  wn_param_offset() is the single source of truth for the offsets.
 */
#ifndef WAVENET_HIP_H_
#define WAVENET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#include "wavenet_hip_gemm.h" /* struct WnGemmArgs of wn_op_gemm */

#ifdef __cplusplus
extern "C" {
#endif

#define WN_ABI_VERSION 22

/* Same fields as the constructor WaveNet(n_quantize, n_aux, n_resch, n_skipch, dilation_depth,
 * dilation_repeat, kernel_size, upsampling_factor)  -- reference wavenet.py:172-173. */
typedef struct WnConfig {
    int32_t n_quantize;
    int32_t n_aux;
    int32_t n_resch;
    int32_t n_skipch;
    int32_t dilation_depth;
    int32_t dilation_repeat;
    int32_t kernel_size;
    int32_t upsampling_factor; /* 0 = no upsampling layer (h arrives at sample rate) */
    int32_t out_channels;      /* channels of conv_post_2; 0 = n_quantize (the reference's softmax head).  A mixture-of-
                                * logistics head uses 3 * n_mixture (BASELINE configs[3]); the front end stays the
                                * n_quantize-class one-hot causal conv */
} WnConfig;

/* Tensor kinds for wn_param_offset (reference state_dict key in the comment). */
enum {
    WN_P_CAUSAL_W = 0, /* causal.conv.weight        (R,Q,K)   wavenet.py:189 */
    WN_P_CAUSAL_B,     /* causal.conv.bias          (R)                      */
    WN_P_UP_W,         /* upsampling.conv.weight    (1,1,1,U) wavenet.py:136 */
    WN_P_UP_B,         /* upsampling.conv.bias      (1)                      */
    WN_P_DSIG_W,       /* dil_sigmoid.l.conv.weight (R,R,K)   wavenet.py:201 */
    WN_P_DSIG_B,       /* dil_sigmoid.l.conv.bias   (R)                      */
    WN_P_DTANH_W,      /* dil_tanh.l.conv.weight    (R,R,K)   wavenet.py:202 */
    WN_P_DTANH_B,      /* dil_tanh.l.conv.bias      (R)                      */
    WN_P_ASIG_W,       /* aux_1x1_sigmoid.l.weight  (R,A,1)   wavenet.py:203 */
    WN_P_ASIG_B,       /* aux_1x1_sigmoid.l.bias    (R)                      */
    WN_P_ATANH_W,      /* aux_1x1_tanh.l.weight     (R,A,1)   wavenet.py:204 */
    WN_P_ATANH_B,      /* aux_1x1_tanh.l.bias       (R)                      */
    WN_P_SKIP_W,       /* skip_1x1.l.weight         (S,R,1)   wavenet.py:205 */
    WN_P_SKIP_B,       /* skip_1x1.l.bias           (S)                      */
    WN_P_RES_W,        /* res_1x1.l.weight          (R,R,1)   wavenet.py:206 */
    WN_P_RES_B,        /* res_1x1.l.bias            (R)                      */
    WN_P_POST1_W,      /* conv_post_1.weight        (S,S,1)   wavenet.py:209 */
    WN_P_POST1_B,      /* conv_post_1.bias          (S)                      */
    WN_P_POST2_W,      /* conv_post_2.weight        (Q,S,1)   wavenet.py:210 */
    WN_P_POST2_B,      /* conv_post_2.bias          (Q)                      */
    WN_P_NKINDS
};

/* flags for wn_forward */
#define WN_FLAG_NO_FUSED 1 /* force the any-size layered path even when the fused R=64 kernels apply */
#define WN_FLAG_EXACT_MFMA 2 /* every contraction on the exact f32-input MFMA (default: the skip-sum / post-net
                              * contractions run on the bf16 matrix cores with a 3-way operand split whose six
                              * products reproduce fp32 to round-off; csrc/wn_gemm6.hip) */
/* Opt-in stream-overlap modes (fused kernels' data chain on the caller's stream, independent contractions on an
 * internal low-priority side stream, fork/join with events inside the call; the caller sees plain stream semantics).
 * Measured on MI355X they do not pay today (the persistent chain kernels hold every wave slot, so a
 * concurrent contraction either starves them or waits), hence not the default; per-launch profiling
 * (wn_prof_enable) always runs serially. */
#define WN_FLAG_BWD_OVERLAP 4 /* wn_backward: weight-gradient contractions on the side stream beside the gate'/dX chain;
                               * same kernels, same reduction order: bit-identical to the serial mode for the same
                               * launch-group size */
#define WN_FLAG_AUX_FUSED 32  /* wn_backward (fused split kernels, upsampling_factor % 16 == 0): the gate kernel also writes the
                               * partial sums of the aux-path gradients (frame-rate aux gradient, upsampling weight), a
                               * small kernel finishes them and dP is not re-read by wn_aux_bwd.  What WaveNetEngine passes by
                               * default since round 2 (measured -3 %); a flag of the C ABI because the sums re-associate
                               * (~1e-7 relative) */
#define WN_FLAG_NO_CHAIN 64   /* wn_backward (fused split kernels, kernel_size <= 2): since ABI v4 the data chain runs as ONE launch
                               * per layer (dX_l and gate'_{l-1} fused, the skip part of dZ pre-contracted for all layers by
                               * one matrix-bound launch; csrc/wn_fused.hip k_chain64s).  This flag restores the former
                               * gate' + dX launch pair per layer (kept for A/B measurements and as an independent check) where
                               * its gate' kernel holds a layer's skip weights (n_skipch <= 352); ignored beyond */
#define WN_FLAG_BWD_OVERLAP_HEAD 16 /* with WN_FLAG_BWD_OVERLAP: only the post-net / skip weight gradients run on the side
                               * stream; the per-layer groups stay on the caller's stream */
#define WN_FLAG_FWD_OVERLAP 8 /* wn_forward (fused kernels): the skip-sum contraction is issued in three chunks of layers on
                               * the side stream while the residual stack is still running (the partial sums round
                               * differently from the single contraction: ~1e-7 relative on the logits) */
#define WN_FLAG_WS_FINITE (1 << 16) /* wn_forward_loss (since ABI v7): the caller vouches that the workspace holds only FINITE
                               * values (it was allocated zero-filled, or an earlier full wn_forward of the same shape wrote it).
                               * wn_forward_loss runs the skip-sum / post-net over the loss window only and leaves the columns
                               * of relu(skip) / relu(post1) in front of it untouched; without this flag it zero-fills them
                               * (two small fills per call) so that a later wn_backward with an earlier window start cannot
                               * multiply dlogits == 0 with NaN / Inf bit patterns of uninitialised memory */
#define WN_FLAG_REPACK (1 << 17)    /* wn_backward / wn_backward_window (since ABI v7): re-build the re-laid-out / pre-split weight
                               * sets in the workspace from the `params` given to THIS call before using them (for callers that
                               * modified params after the forward call; costs one pack pass, ~0.05 ms at the BASELINE size) */
#define WN_FLAG_DW_3PRODUCT (1 << 18) /* wn_backward / wn_backward_window (since ABI v8, opt-in): the weight-gradient contractions -- LEAF results:
                               * sums over every position of the minibatch that no other layer consumes -- take three of the six
                               * products of the 3-way operand split (h h + h m + m h; two bf16 pieces per operand: relative error
                               * ~2^-16 per product, random in sign, instead of 2^-24).  Never applied to a contraction whose
                               * output feeds another layer.  Default off: every contraction fp32-equivalent. */
#define WN_FLAG_DW_F16PAIR (1 << 19) /* wn_backward / wn_backward_window (since ABI v8; opt-in at this boundary, where flags = 0 means six
                               * bf16 products everywhere -- the Python engine sets it by default): the weight-gradient contractions split
                               * their operands into TWO fp16 pieces (11 + 11 significand bits) and take the three products
                               * h h + h l + l h on v_mfma_f32_32x32x16_f16: ~2^-22 relative per product -- below the rounding of an
                               * fp32 running sum over a minibatch's positions -- at half the matrix work of the six bf16 products.
                               * fp16 has 5 exponent bits, so the SIZE of the gradient decides the scale: the gradient operand of
                               * every weight-gradient contraction is multiplied by 2^(e + WN_DW_F16_HEADROOM) before the split and
                               * the result by its inverse (activations are taken as they are), where 2^-e bounds max |dlogits|.
                               * Since ABI v9 the library MEASURES that maximum (a bound that is merely safe -- the a-priori
                               * grad_scale / positions of a mean cross-entropy on a well-fitted model, a forgotten exponent -- would
                               * push the scaled operand into fp16's subnormals and silently cost precision):
                               *   WN_FLAG_DW_F16PAIR alone                      one pass over the `dlogits` given to this call (its loss
                               *                                                  window; ~35 us at the BASELINE size) finds the maximum
                               *   | WN_FLAG_DW_F16_AMAX_WS                       the caller vouches that `dlogits` is, unmodified, what the
                               *                                                  last wn_forward_loss / wn_softmax_ce_loss call ON THIS
                               *                                                  WORKSPACE wrote: those calls leave its maximum in the
                               *                                                  workspace (their epilogue computes it for free)
                               *   | WN_FLAG_DW_F16_EXP_VALID | WN_FLAG_DW_F16_EXP(e)   the caller's own promise max |dlogits| <= 2^-e
                               *                                                  (0 <= e <= 63), taken as given (v8 took the exponent
                               *                                                  field without a valid bit: e = 0 was a silent default)
                               * The scale is decided on the device (no host synchronisation).  Values down to 2^-(e+11) keep all 22
                               * bits.  A back-propagated gradient more than 2^(16 - WN_DW_F16_HEADROOM) times the maximum leaves fp16's
                               * range: the launch detects it (non-finite result) and a six-product launch issued right behind every
                               * fp16 launch, which otherwise returns at once, redoes the contraction -- the result is then the
                               * default mode's; the same redo is forced when no usable maximum exists (all-zero or non-finite
                               * gradient, WN_FLAG_DW_F16_AMAX_WS without such a loss call).  Wins over WN_FLAG_DW_3PRODUCT. */
#define WN_FLAG_DW_F16_EXP_SHIFT 20
#define WN_FLAG_DW_F16_EXP(e) (((e) & 63) << WN_FLAG_DW_F16_EXP_SHIFT)
#define WN_DW_F16_HEADROOM 8
#define WN_FLAG_DW_F16_EXP_VALID (1 << 26) /* since ABI v9: the WN_FLAG_DW_F16_EXP(e) field is the caller's promise (e = 0 included) */
#define WN_FLAG_DW_F16_AMAX_WS (1 << 27)   /* since ABI v9: max |dlogits| as the last loss call of this workspace measured it */
#define WN_FLAG_MM_F16PAIR (1 << 28) /* since ABI v9, opt-in: wn_forward / wn_forward_loss / wn_backward(_window) -- the weights x activations
                               * contractions on the split matrix-core kernel (skip sum, post-net, their data gradients, the per-layer
                               * contractions of wide models) take the fp16 pair split too (two fp16 pieces per operand, three products,
                               * ~2^-22 per product: the rounding of an fp32 running sum over >= 64 terms) instead of the six bf16
                               * products.  Activations are taken as they are, back-propagated gradients scaled by the measured maximum
                               * like the weight gradients' (the same three sources, see WN_FLAG_DW_F16PAIR); every such launch is
                               * followed by a conditional six-product launch that redoes it if an operand left fp16's range.  The same
                               * flag must be given to the forward and the backward call of a step (the workspace holds the weight
                               * images the forward call packed), or wn_backward gets WN_FLAG_REPACK. */
#define WN_FLAG_FUSED_F16PAIR (1 << 29) /* since ABI v9, opt-in: wn_forward / wn_forward_loss -- the fused 64-channel residual block (taps, gate, res
                               * 1x1) on the fp16 pair split as well (three products per multiply instead of six), BLOCK-SCALED: every
                               * weight image and every 64 x 32 operand tile is multiplied by the power of two that puts its maximum
                               * at 2^12 / 2^14, so no magnitude can leave fp16's range and no redo is needed (csrc/wn_fused.hip
                               * k_resblock_fwd<K, FwdF16x2>).  Forward only: the backward chain keeps six bf16 products. */
#define WN_FLAG_CHAIN_F16PAIR (1 << 30) /* since ABI v9, opt-in: wn_forward(_loss) packs and wn_backward(_window) uses -- the fused backward data chain
                               * (dX_l from dP_l, gate' of layer l-1) on the block-scaled fp16 pair split (k_chain64s<.., H16>): weight
                               * images by the power of two of their maximum, the dP operand of a tile by the maximum of the producer
                               * tiles it reads (every chain launch records max |dP| per 32-sample tile beside dP), the dX operand by
                               * its own maximum.  Same flag for the forward and the backward call of a step (the images are packed by
                               * the forward call), or WN_FLAG_REPACK. */
#define WN_FLAG_DW_FLUSH(n) (((n) & 0xff) << 8) /* wn_backward: issue the weight gradients of at most n walked layers per
                               * launch group (0 = default: a whole gradient bucket; 5 layers with WN_FLAG_BWD_OVERLAP).
                               * Groups never straddle a bucket.  The split-K plan of a group depends on its size, so
                               * different n round differently (~1e-7 relative) */

int wn_abi_version(void);
const char* wn_last_error(void);

/* receptive_field = (K-1)*sum(dilations)+1, dilations = [2^i for i<depth]*repeat (wavenet.py:184-185) */
int wn_receptive_field(const WnConfig* cfg);
int wn_num_layers(const WnConfig* cfg);

/* Number of fp32 elements of the flat parameter buffer (== sum of numel of the reference state_dict);
 * -1 for an invalid configuration (wn_last_error() says which field). */
int64_t wn_param_count(const WnConfig* cfg);
/* Offset (in floats) and numel of tensor `kind` of layer `layer` (ignored for non per-layer kinds)
 * inside the flat parameter / gradient buffers.  Returns non-zero if the tensor does not exist
 * (upsampling tensors when upsampling_factor == 0). */
int wn_param_offset(const WnConfig* cfg, int kind, int layer, int64_t* offset, int64_t* numel);

/* Gradient buckets for data-parallel all-reduce: bucket 0 = post-net + all skip_1x1; then groups of
 * `layers_per_bucket` residual layers from the last layer down; the final bucket = causal +
 * upsampling.  With ONE layer group (layers_per_bucket <= 0 or >= the number of layers) the skip_1x1
 * tensors belong to that group's bucket instead (bucket 0 = post-net only): their gradients may then
 * be produced behind the data chain, together with the res_1x1 gradients.  The buckets are contiguous,
 * disjoint and cover the buffer; [lo, hi) are float offsets into the flat gradient buffer. */
int wn_num_buckets(const WnConfig* cfg, int layers_per_bucket);
int wn_bucket_range(const WnConfig* cfg, int layers_per_bucket, int bucket, int64_t* lo, int64_t* hi);
/* [lo, hi) of parameters that never receive a gradient (res_1x1 of the last layer; reference:
 * wavenet.py:231-238 leaves its output unused, so torch reports grad None and Adam skips it). */
int wn_dead_param_range(const WnConfig* cfg, int64_t* lo, int64_t* hi);

/* Bytes of caller-provided scratch for batch B x T model inputs (forward + backward); 0 for an invalid
 * configuration or shape (wn_last_error()).
 * No entry point reads a word of the workspace that was not written earlier in the same call or in the forward / loss call the
 * backward call belongs to, so nothing depends on what the buffer held before: a buffer of at least this size may be reused
 * from step to step, across (B, T) shapes (size it for the largest) and across flag sets, without clearing it in between.  The
 * two assumptions on earlier contents are opt-in flags: WN_FLAG_WS_FINITE (wn_forward_loss) and WN_FLAG_DW_F16_AMAX_WS
 * (wn_backward: the maximum the last loss call on THIS workspace left).  tests/workspace_common.py holds the library to this. */
size_t wn_workspace_bytes(const WnConfig* cfg, int B, int T);

/* Introspection for parity tests (since ABI v4; the training path never calls it): offset and length, in floats, of
 * a tensor that wn_forward / wn_backward leave in the workspace of a (B, T) call.  Layouts (time contiguous):
 *   X, SIGMOID, TANH, Z  (L, B, R, T)  layer input x_l, sigmoid(.) and tanh(.) of the gate, z_l = their product
 *                                      (reference wavenet.py:525-536; x_0 = the front conv's output).  TANH is only
 *                                      written by the any-size kernels: the fused n_resch = 64 kernels save the sigmoid
 *                                      half and z, and rebuild tanh = z / sigmoid in the backward pass
 *   RELU_SKIP, RELU_POST1 (B, S, T)    relu(sum of skips), relu(conv_post_1(.))  (wavenet.py:519-521): their
 *                                      positivity is the ReLU sub-gradient wn_backward uses
 *   DSKIP (B, S, T), DP (L, B, 2R, T), DX (L, B, R, T)   after wn_backward: dL/d(skip sum), dL/d(gate pre-activations
 *                                      [sigmoid rows ; tanh rows]), dL/dx_l */
enum { WN_WS_X = 0, WN_WS_SIGMOID = 1, WN_WS_TANH = 2, WN_WS_Z = 3, WN_WS_RELU_SKIP = 4, WN_WS_RELU_POST1 = 5,
       WN_WS_DSKIP = 6, WN_WS_DP = 7, WN_WS_DX = 8 };
int wn_workspace_region(const WnConfig* cfg, int B, int T, int kind, int64_t* offset_floats, int64_t* n_floats);

/* WaveNet.forward(x, h)  -- reference wavenet.py:212-241 (+ _preprocess :513-516, UpSampling
 * :141-154, _residual_forward :525-536, _postprocess :518-523).
 *   params : flat parameter buffer                         (device, wn_param_count floats)
 *   x      : (B, T) int64 sample indices, taken modulo n_quantize like OneHot (wavenet.py:88)
 *   h      : (B, n_aux, T / upsampling_factor) fp32, or (B, n_aux, T) when upsampling_factor == 0
 *   logits : (B, n_quantize, T) fp32 out  [view it as (B, T, Q) via transpose(1,2)]
 * Everything the backward pass needs is kept in `ws`. */
int wn_forward(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
               float* logits, void* ws, size_t ws_bytes, int flags, void* stream);

/* nn.CrossEntropyLoss()(out[:, t_start:].reshape(-1,Q), target[:, t_start:].reshape(-1))
 *   -- reference train.py:461,534-536 (t_start = receptive_field there).
 *   loss     : device scalar out = mean over B*(T-t_start) positions, times loss_scale
 *   dlogits  : (B, Q, T) out = d(mean loss)/d(logits) * grad_scale  (zeros for t < t_start); may be NULL */
int wn_softmax_ce_loss(const WnConfig* cfg, int B, int T, const float* logits, const int64_t* target, int t_start,
                       float grad_scale, float loss_scale, float* loss, float* dlogits, void* ws, size_t ws_bytes,
                       void* stream);

/* wn_forward + wn_softmax_ce_loss in one call, for the training step (since ABI v5; reference train.py:533-536:
 * batch_output = model(x, h); loss = CrossEntropyLoss()(batch_output[:, rf:], batch_t[:, rf:])).  When
 * wn_forward_loss_fused(cfg, B, T, flags) == 1 the loss is the EPILOGUE of the conv_post_2 contraction: a workgroup holds all
 * n_quantize <= 256 classes of its 128 positions on chip, so the (B, Q, T) logits are never written to or read back from
 * memory -- `loss` and `dlogits` (nullable) come out exactly as wn_softmax_ce_loss defines them, logits_scratch is not
 * touched (may be NULL).  Otherwise (exact-MFMA mode, more than 256 classes, mixture head) the call runs the two entry
 * points back to back and needs logits_scratch (B, Q, T).
 * Workspace after the call: as wn_forward leaves it, EXCEPT that the fused form computes the skip sum and the post-net over
 * the loss window only -- columns [t0, T) with t0 = t_start rounded down to a multiple of 128: relu(skip) and relu(post1)
 * (WN_WS_RELU_SKIP / WN_WS_RELU_POST1) are valid from t0 on; in front of t0 they hold zeros (or, with WN_FLAG_WS_FINITE,
 * whatever finite values were there).  dlogits is exactly zero there, so a backward pass over ANY window start t_first <= t_start
 * (wn_backward included) yields the same gradients; wn_backward_window(t_first = t_start) is the cheapest. */
int wn_forward_loss_fused(const WnConfig* cfg, int B, int T, int flags);
int wn_forward_loss(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                    const int64_t* target, int t_start, float grad_scale, float loss_scale, float* loss, float* dlogits,
                    float* logits_scratch, void* ws, size_t ws_bytes, int flags, void* stream);

/* The loss of a PADDED batch of sequences of unequal length (since ABI v11; additions only): wn_softmax_ce_loss and
 * wn_forward_loss with a per-sequence end.  It is nn.CrossEntropyLoss() -- the reference's own loss object, train.py:461 -- on
 * [:, t_start:] with the targets set to its default ignore_index (-100) from t_end[b] on:
 *   t_end   : (B,) int32 on the DEVICE, 1 <= t_end[b] <= T: sequence b carries loss on the positions [t_start, t_end[b]);
 *             a sequence with t_end[b] <= t_start carries none.  NULL = T for every sequence: the dense entry point, bit for bit.
 *   n_loss  : N = sum_b max(t_end[b] - t_start, 0), counted by the CALLER on the host (the lengths are host integers, so the
 *             step gains no device-to-host synchronisation); the library does not read t_end back to check it.
 *             n_loss <= 0, n_loss > B * (T - t_start), and t_end == NULL with n_loss != B * (T - t_start) are errors.
 *   loss    = loss_scale * (sum of the per-position losses over the loss positions) / N
 *   dlogits = grad_scale / N * d(sum)/d(logits) on the loss positions and EXACTLY 0.0f on every other position, the padding
 *             included -- so the backward entry points need no lengths: wn_backward_window / wn_backward_dh with
 *             t_first = t_start contract zeros there, every parameter gradient is that of the valid positions alone, and
 *             dh is exactly zero on frames wholly behind a sequence's end (the network is causal).
 * The padding -- x, h, target behind t_end[b] -- may hold anything finite; targets there are still read modulo n_quantize,
 * they carry no loss.  The fused form is taken exactly where the dense entry point takes it (wn_forward_loss_fused); the
 * residual stack and the backward pass still compute every position of the (B, T) rectangle. */
int wn_softmax_ce_loss_ragged(const WnConfig* cfg, int B, int T, const float* logits, const int64_t* target, int t_start,
                              const int32_t* t_end, int64_t n_loss, float grad_scale, float loss_scale, float* loss,
                              float* dlogits, void* ws, size_t ws_bytes, void* stream);
int wn_forward_loss_ragged(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                           const int64_t* target, int t_start, const int32_t* t_end, int64_t n_loss, float grad_scale,
                           float loss_scale, float* loss, float* dlogits, float* logits_scratch, void* ws, size_t ws_bytes,
                           int flags, void* stream);

/* Knowledge distillation (since ABI v18; additions only): the softmax head's loss against a teacher's distribution.  For every
 * loss position (t_start <= t < t_end[b], as wn_softmax_ce_loss_ragged) with s the student's and u the teacher's logit column,
 * y = target mod n_quantize, P = softmax(u / tau), S = softmax(s / tau):
 *   ce = logsumexp(s) - s_y,   kl = sum_q P_q (log P_q - log S_q)  (a class with P_q == 0 adds exactly 0; not clamped)
 *   l  = (1 - alpha) ce + alpha tau^2 kl                            (Hinton's form: tau^2 keeps the gradient's scale)
 *   loss[0] = loss_scale / N * sum l,  loss[1] = loss_scale / N * sum ce,  loss[2] = loss_scale / N * sum kl (unweighted)
 *   dlogits_q = grad_scale / N * ((1 - alpha) (softmax(s)_q - [q == y]) + alpha tau (S_q - P_q)), EXACTLY 0.0f off the loss
 *   positions.  The teacher is a constant: nothing is differentiated with respect to u.
 *   teacher_logits : (B, n_quantize, T) fp32, the layout wn_forward writes
 *   alpha in [0, 1], tau > 0 and finite.  alpha == 1: target is not read (may be NULL) and ce is 0; alpha == 0: l = ce.
 *   loss     : THREE floats on the device
 *   dlogits  : nullable; pos_loss : nullable, (B, T) out = l per position, unscaled, 0 off the loss positions.  The loss bits do
 *              not depend on whether either is given.
 *   scratch  : wn_softmax_distill_scratch_floats(B, T) floats on the device; holds the per-block partial sums, which are added
 *              in a fixed order (no atomics: the same inputs give the same bits).  Nothing is read from it, or from the
 *              workspace, that the call did not write: the result does not depend on what either held before.
 * The workspace keeps its size and layout; the call leaves max |dlogits| in the word the other loss calls use, so a backward
 * call may take WN_FLAG_DW_F16_AMAX_WS.  Two plain launches on `stream`.  A mixture-of-logistics model (out_channels > 0),
 * alpha or tau out of range, a NULL among logits / teacher_logits / target (alpha < 1) / loss / scratch and the n_loss
 * conditions of the ragged entry points are errors: no launch is made. */
int64_t wn_softmax_distill_scratch_floats(int B, int T);
int wn_softmax_distill_loss(const WnConfig* cfg, int B, int T, const float* logits, const float* teacher_logits,
                            const int64_t* target, int t_start, const int32_t* t_end, int64_t n_loss, float alpha, float tau,
                            float grad_scale, float loss_scale, float* loss, float* dlogits, float* pos_loss, float* scratch,
                            void* ws, size_t ws_bytes, void* stream);

/* Weighted cross-entropy (since ABI v19; additions only): the softmax head's criterion with one weight per class, label
 * smoothing and one weight per position.  For every loss position i = (b, t) (t_start <= t < t_end[b], as
 * wn_softmax_ce_loss_ragged) with s the logit column, y = target mod n_quantize, p = softmax(s), w = class_weights (NULL: ones),
 * r = pos_weights (NULL: ones), Q = n_quantize, W = sum_q w_q:
 *   ce_i = -log p_y
 *   l_i  = (1 - eps) w_y ce_i + (eps / Q) sum_q w_q (-log p_q)      (a class with w_q == 0 adds exactly 0; not clamped)
 *   g_iq = (1 - eps) w_y (p_q - [q == y]) + (eps / Q) (W p_q - w_q)
 *   D    = sum_i r_i w_{y_i}  (normalize == 0, "weights": torch's mean reduction)  or  n_loss  (normalize == 1, "positions")
 *   loss[0] = loss_scale * sum_i r_i l_i / D   -- the criterion; with r == NULL and normalize == 0 this is
 *             torch.nn.functional.cross_entropy(s, y, weight=w, label_smoothing=eps)
 *   loss[1] = loss_scale * sum_i ce_i / n_loss -- the plain unweighted cross-entropy of the same positions
 *   loss[2] = D
 *   dlogits_iq = grad_scale * r_i g_iq / D, EXACTLY 0.0f off the loss positions and where r_i == 0
 *   pos_loss_i = r_i l_i (nullable, (B, T) out), 0 off the loss positions and where r_i == 0
 * One deviation from torch: D == 0 gives loss[0] = 0 and dlogits = 0 exactly (torch: NaN).  A position with r_i == 0 is off: it
 * adds 0 whatever its column holds.  Otherwise nothing is clamped: a -inf logit with eps > 0 and w_q > 0 gives l = +inf as in
 * torch, a NaN or +inf stays in its column.
 *   class_weights : nullable, (n_quantize,) fp32 on the device; pos_weights : nullable, (B, T) fp32 on the device.  Every weight
 *                   finite and >= 0: the caller's contract, not checked here.
 *   eps in [0, 1); normalize 0 or 1.  With "positions" and per-call shares n_loss_k / sum n_loss of grad_scale the objective
 *   pooled over ranks and micro-batches is exact; with "weights" it is the share-weighted mean of per-call weighted means.
 *   loss    : THREE floats on the device
 *   dlogits : nullable; pos_loss : nullable.  The loss bits do not depend on whether either is given.
 *   scratch : wn_softmax_cew_scratch_floats(B, T) floats on the device, 8-byte aligned; holds D, 1 / D and the per-block
 *             partial sums, which are added in a fixed order (no atomics, no host synchronisation: the same inputs give the
 *             same bits).  Nothing is read from it, or from the workspace, that the call did not write.
 * The workspace keeps its size and layout; the call leaves max |dlogits| in the word the other loss calls use, so a backward
 * call may take WN_FLAG_DW_F16_AMAX_WS.  Two plain launches on `stream`, four when D has to be summed on the device
 * (normalize == 0 with a weight of either kind).  A mixture-of-logistics model (out_channels > 0), eps outside [0, 1), another
 * normalize, a NULL among logits / target / loss / scratch, a misaligned scratch and the n_loss conditions of the ragged entry
 * points are errors: no launch is made. */
int64_t wn_softmax_cew_scratch_floats(int B, int T);
int wn_softmax_cew_loss(const WnConfig* cfg, int B, int T, const float* logits, const int64_t* target, int t_start,
                        const int32_t* t_end, int64_t n_loss, const float* class_weights, const float* pos_weights, float eps,
                        int normalize, float grad_scale, float loss_scale, float* loss, float* dlogits, float* pos_loss,
                        float* scratch, void* ws, size_t ws_bytes, void* stream);

/* Scoring held-out data (since ABI v13; additions only): the negative log-likelihood of each sequence of a batch, without a
 * gradient and without a divisor.
 *   row_nll : (B,) fp32 out on the device: row_nll[b] = SUM of the per-position negative log-likelihoods of sequence b over
 *             the positions [t_start, min(t_end[b], T)).  A sum, not a mean: the caller knows the counts, and sums pool
 *             exactly over batches of any size.  A sequence with no position in that range gets exactly 0.0f, and a batch in
 *             which no sequence has one succeeds (t_start >= T included).  NULL is an error.
 *   t_end   : (B,) int32 on the device, or NULL = T for every sequence (as wn_forward_loss_ragged).
 *   acc     : nullable, ONE double on the device: acc[0] += the fp64 sum of row_nll as returned (the rows rounded to fp32,
 *             added in double in ascending order), so the total of a pass is the sum of its per-sequence results.  A pass
 *             over many batches accumulates there and the host reads it once.
 * Each row is added in double in an order that depends on the number of column blocks alone and rounded to fp32 once; no atomics:
 * the same inputs give the same bits.  The result does not depend on what the workspace held before the call, with or without
 * WN_FLAG_WS_FINITE; the calls leave the workspace's max |dlogits| word alone, and the workspace afterwards is NOT an input
 * of the backward entry points.
 *   wn_forward_nll      : wn_forward_loss without dlogits (softmax head); logits_scratch (B, Q, T) is needed exactly where
 *                         wn_forward_loss_fused(cfg, B, T, flags) == 0, NULL otherwise.
 *   wn_softmax_nll_rows : the same rows from logits (B, Q, T) that already exist.
 *   wn_mol_nll_rows     : the mixture-of-logistics head, from out (B, 3 * n_mix, T) of wn_forward and the waveform y (B, T);
 *                         num_classes / log_scale_min as wn_mol_loss. */
int wn_forward_nll(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                   const int64_t* target, int t_start, const int32_t* t_end, float* row_nll, double* acc,
                   float* logits_scratch, void* ws, size_t ws_bytes, int flags, void* stream);
int wn_softmax_nll_rows(const WnConfig* cfg, int B, int T, const float* logits, const int64_t* target, int t_start,
                        const int32_t* t_end, float* row_nll, double* acc, void* ws, size_t ws_bytes, void* stream);
int wn_mol_nll_rows(const WnConfig* cfg, int B, int T, const float* out, const float* y, int t_start, const int32_t* t_end,
                    int num_classes, float log_scale_min, float* row_nll, double* acc, void* ws, size_t ws_bytes, void* stream);
/* The reduction behind them on its own (op level): row_out[b] = sum of partial[b * nblk .. (b + 1) * nblk), one workgroup.
 * Here acc[0] += the sum of the row sums as they are in DOUBLE, before their rounding to fp32, rows in ascending order. */
int wn_op_row_sums(const float* partial /*[B][nblk]*/, int B, int nblk, float* row_out /*B*/, double* acc /*nullable*/,
                   void* stream);

/* Backward of wn_forward (what autograd does for train.py:538): writes EVERY element of the flat
 * gradient buffer `grads` (the dead range gets zeros).  `ws` must still hold the matching
 * wn_forward call, made with the same WN_FLAG_NO_FUSED / WN_FLAG_EXACT_MFMA choice (the two kernel
 * families save different activations), and `params` must be UNCHANGED since that call: the workspace also holds the
 * re-laid-out / pre-split weight sets wn_forward packed from them (the post-net and skip weights of the backward
 * contractions among them), and wn_backward does not re-pack unless WN_FLAG_REPACK is given.  The training loop satisfies
 * this by construction (the optimizer step comes after the backward pass, train.py:533-539); the Python engine tracks a
 * parameter version and raises, like torch.autograd does for a tensor modified in place between forward and backward.  If events != NULL, hipEvent_t events[i] is recorded on
 * `stream` as soon as bucket i (wn_bucket_range) is final, so the caller can all-reduce it on another stream. */
int wn_backward(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                const float* dlogits, float* grads, void* ws, size_t ws_bytes, void* const* events, int n_events,
                int layers_per_bucket, int flags, void* stream);

/* wn_backward for a loss that covers positions [t_first, T) only (since ABI v5) -- the reference's training loss,
 * train.py:534-536: CrossEntropyLoss on batch_output[:, receptive_field:].  The caller guarantees
 * dlogits[:, :, :t_first] == 0 (wn_softmax_ce_loss / wn_mol_loss with t_start = t_first write exactly that).  Between the
 * logits and the residual stack everything is pointwise in time (wavenet.py:518-523,533), so dO2, dSkip and the skip part
 * of every layer's dZ are zero in front of t_first as well: their contractions and the post-net / skip weight gradients
 * run over the window only (from t_first rounded down to a multiple of 128; the skipped columns of dSkip are zero-filled
 * for the residual chain, which needs every position).  Same gradients as wn_backward up to the rounding of a different
 * split-K plan; t_first = 0 IS wn_backward. */
int wn_backward_window(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                       const float* dlogits, int t_first, float* grads, void* ws, size_t ws_bytes, void* const* events,
                       int n_events, int layers_per_bucket, int flags, void* stream);

/* wn_backward_window plus the gradient with respect to the aux features (since ABI v10): dh[b][a][f] = dL/dh, (B, n_aux, F)
 * contiguous like h (F = T / upsampling_factor, or T without the upsampling layer), scaled like the weight gradients.
 *   with the upsampling layer:  dh[b][a][f] = sum_l sum_c Waux_l[c][a] * dG_l[b][c][f],  dG_l[b][c][f] = sum_j w_up[j] dP_l[b][c][fU + j]
 *   without it:                 dh[b][a][t] = sum_l sum_c Waux_l[c][a] * dP_l[b][c][t]
 * (c: the 2 n_resch rows of aux_1x1_sigmoid then aux_1x1_tanh; the biases do not enter).  ONE contraction over all layers
 * (K = L * 2 n_resch) on the fp32-input matrix cores after the last weight-gradient group, on its stream: exact fp32 products,
 * every element a fixed-order sum -- the same bits on every call and under every launch plan that leaves dP itself unchanged.
 *   dh == NULL:    exactly wn_backward_window (same launches, same results).
 *   grads == NULL: a frozen model -- only what dh needs runs (the data chain, the post-net data gradients, dG); no weight
 *                  gradient, no reduction of one and no scale scan for one (WN_FLAG_MM_F16PAIR keeps the one of its data
 *                  contractions).  Requires dh != NULL and events == NULL, n_events == 0.
 * Same workspace (wn_workspace_bytes) as wn_backward; the x gradient is not defined (x holds class indices). */
int wn_backward_dh(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                   const float* dlogits, int t_first, float* grads, float* dh, void* ws, size_t ws_bytes, void* const* events,
                   int n_events, int layers_per_bucket, int flags, void* stream);

/* wn_backward_dh for a model with frozen parameters (since ABI v16): the pass stops where no trainable parameter needs it.
 *   first_layer   the lowest layer l whose own tensors (dil_*, aux_1x1_*, skip_1x1.l, res_1x1.l) include a trainable one; L when
 *                 no layer tensor trains.  It must be 0 when dh != NULL, or when the front conv or the upsampling layer trains
 *                 (both need every layer's data gradient) -- an error otherwise.
 *   needs         WN_NEED_POST | WN_NEED_FRONT | WN_NEED_UP: the post-net, the front conv, the upsampling layer train.
 * What is left out: the post-net weight gradients without WN_NEED_POST (and the two data contractions in front of them when
 * first_layer == L as well); the data chain below first_layer, including the launch that would produce dX_{first_layer}
 * (kept for first_layer == 0 with WN_NEED_FRONT); the weight-gradient groups below first_layer -- groups are counted from the top
 * as in the full pass, so a group wholly at or above first_layer issues the full pass's launches with its split-K plan, and the
 * lowest one is cut at first_layer; the front-conv gradient and the upsampling reductions without their bits.  The two
 * all-layers contractions (the skip part of dZ, and skip_1x1 where it is one launch) keep all L layers while any layer is
 * computed and fall away with first_layer == L: their plans follow the row / column count, and the computed layers keep the
 * full pass's bits this way.  Nothing is left out inside a computed layer.  Every bucket event is still
 * recorded, in order (a bucket whose layers were all left out: where the walk would have reached it).
 * The gradient buffer: ranges of tensors outside what was asked for hold UNSPECIFIED values (written or not).
 * first_layer = 0 with WN_NEED_ALL is wn_backward_dh, launch for launch. */
#define WN_NEED_POST 1
#define WN_NEED_FRONT 2
#define WN_NEED_UP 4
#define WN_NEED_ALL 7
int wn_backward_needs(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                      const float* dlogits, int t_first, float* grads, float* dh, void* ws, size_t ws_bytes, void* const* events,
                      int n_events, int layers_per_bucket, int flags, void* stream, int first_layer, int needs);

/* torch.optim.Adam step over the flat buffers (reference train.py:457-460,539): L2-in-gradient
 * weight decay, bias correction with `step` (1-based); [skip_lo, skip_hi) is left untouched. */
int wn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int64_t skip_lo, int64_t skip_hi,
                 void* stream);

/* ---- global-norm gradient clipping and the non-finite-step guard (since ABI v12) ----
 * Device-resident state of the guarded optimizer step: 56 bytes, 8-byte aligned, owned by the caller (zero it once; the two
 * step counters are the only words that carry over from call to call, everything else is rewritten by every wn_grad_norm).
 * Nothing here is read by the host on the training path: the Adam launch takes its scalars from this block. */
typedef struct WnOptState {
    double sumsq;          /*  0: sum of grads[i]^2 outside the skip range, accumulated in double */
    float total_norm;      /*  8: (float)sqrt(sumsq): the norm BEFORE clipping (torch's clip_grad_norm_ return value) */
    float clip_coef;       /* 12: min(1, max_norm / (total_norm + 1e-6)) in double, cast; exactly 1 when clipping is off */
    int32_t apply;         /* 16: 1 = the Adam launch updates; 0 = guard on and the gradient is not finite: it writes nothing */
    int32_t reserved;      /* 20: written as 0 */
    int64_t steps_applied; /* 24: STATE: number of applied steps == the `step` of Adam's bias correction */
    int64_t steps_skipped; /* 32: STATE: number of skipped steps */
    float lr_over_bc1;     /* 40: lr / (1 - beta1^steps_applied) of this step (0 when it does not apply) */
    float sqrt_bc2;        /* 44: sqrt(1 - beta2^steps_applied) of this step (0 when it does not apply) */
    float beta1;           /* 48: as given to the norm call */
    float beta2;           /* 52 */
} WnOptState;

/* Floats of scratch the norm needs for a buffer of n elements (one double per block of a grid that depends on n alone). */
int64_t wn_grad_norm_scratch_floats(int64_t n);
/* Two launches on `stream`, no host synchronisation:
 *   1. sum of squares of grads[0, n) without [skip_lo, skip_hi), 16-byte loads with a scalar head / tail (grads needs 4-byte
 *      alignment only), double accumulation per thread, wave and block, one partial per block, no atomics.  The grid is a
 *      function of n alone and every sum has a fixed order: the same buffer (same address modulo 16) gives the same bits on
 *      every device, so data-parallel ranks holding the same reduced gradient derive the same coefficient;
 *   2. one block sums the partials in double and fills `state`: total_norm, clip_coef (max_norm <= 0 or infinite: measure
 *      only, clip_coef = 1), apply, the counters, and lr / bc1 and sqrt(bc2) from the double formulas of the unguarded step
 *      with the device's count of applied steps.
 * Finiteness is judged on the double sum: finite elements of any magnitude never make it non-finite, a NaN or +-inf outside the
 * skip range always does.  guard != 0: a non-finite gradient sets apply = 0, counts a skipped step and leaves the applied count;
 * guard == 0: the step applies whatever the gradient holds (NaN reaches the weights, as in torch).
 * scratch (8-byte aligned) and `state` influence no result through what they held before, the two counters excepted. */
int wn_grad_norm(const float* grads, int64_t n, int64_t skip_lo, int64_t skip_hi, float max_norm, int guard, float lr,
                 float beta1, float beta2, float* scratch, WnOptState* state, void* stream);
/* The Adam step above with lr / bc1, sqrt(bc2), beta1, beta2, clip_coef and apply read from `state` as the preceding norm call
 * on the same stream left them: g = clip_coef * grads[i] BEFORE the weight-decay term (torch clips the raw gradient; the
 * optimizer adds L2 decay afterwards); `grads` itself is NOT modified (it keeps the unclipped values, unlike torch's in-place
 * clip); when apply == 0 nothing is written to params, exp_avg or exp_avg_sq. */
int wn_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float eps,
                         float weight_decay, int64_t skip_lo, int64_t skip_hi, const WnOptState* state, void* stream);

/* ---- exponential moving average of the weights inside the Adam launch (since ABI v14; additions only) ----
 * wn_adam_step / wn_adam_step_guarded with one more flat fp32 buffer `ema` of n elements: params, exp_avg and exp_avg_sq receive
 * exactly the bits of the plain calls, and with the new weight p_new still in a register the same launch does
 *     ema[i] = fmaf(w, p_new - ema[i], ema[i]),    w = (float)(1.0 - d_t), formed in double,
 *     d_t = ema_warmup != 0 ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay.
 * The increment form is the contract: ema == p_new is its exact fixed point, which d * ema + (1 - d) * p_new is not (for d = 0.9999
 * the two fp32 coefficients no longer sum to 1 and the fixed point sits about 3e-4 relative off p).  An increment below half an
 * ulp of ema[i] is lost, as in any fp32 average.
 * t is the 1-based count of APPLIED steps including this one: `step` in wn_adam_step_ema (the host forms w), the state block's
 * steps_applied as the preceding wn_grad_norm left it in wn_adam_step_guarded_ema (every thread forms w from it, with the same
 * double arithmetic: the same t gives the same w bits on both paths).
 * Skip rule: ema[skip_lo, skip_hi) is never written, like the other three buffers.
 * Apply rule (guarded): when state->apply == 0 nothing at all is written -- weights, moments and ema stay, and t does not advance.
 * WnOptState keeps its 56 bytes.  One launch each (the guarded step stays 3 launches with its norm).
 * Errors (wn_last_error): ema == NULL, ema_decay outside [0, 1), ema overlapping params. */
int wn_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, int64_t step,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int64_t skip_lo, int64_t skip_hi,
                     double ema_decay, int ema_warmup, void* stream);
int wn_adam_step_guarded_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float eps,
                             float weight_decay, int64_t skip_lo, int64_t skip_hi, const WnOptState* state, double ema_decay,
                             int ema_warmup, void* stream);

/* ---- training with frozen parameters: the norm and the Adam step over LIVE RANGES (since ABI v16; additions only) ----
 * A model with frozen parameters updates some ranges of its flat buffers and must leave the rest alone -- weights, both moments
 * and the moving average bit for bit, with no weight decay -- whatever the gradient buffer holds there (it may hold anything: a
 * backward pass need not write the gradient of a frozen tensor).  The entry points below are wn_grad_norm, wn_adam_step(_ema) and
 * wn_adam_step_guarded(_ema) with a table of live ranges in the place of the one skip range; the calls above stay as they are.
 *
 * wn_live_table (host only, no launch): `ranges` holds n_ranges pairs lo, hi -- non-empty ranges [lo, hi) inside [0, n), sorted
 * and disjoint (touching ranges are allowed).  It writes the 3 * n_ranges int64 words of the table to `table` (host memory):
 * lo[n_ranges], hi[n_ranges], before[n_ranges] = the number of live elements in front of each range, and returns n_live, the
 * number of live elements; -1 on an error (wn_last_error: NULL, an empty table, an empty range, ranges that are not sorted and
 * disjoint, a range outside [0, n)).  The caller copies the words to device memory (8-byte aligned) once per freeze set; the
 * launching calls take that device copy with n_ranges and n_live, and trust it to be what wn_live_table wrote.
 *
 * The kernels walk the compacted index space [0, n_live) with the grid the whole-buffer kernel would use for n_live elements and
 * map an index to its buffer element through the table (staged in LDS up to 1024 ranges, read from global memory beyond; a
 * thread bisects once and then moves forward).  An element outside every range is neither read nor written in any buffer.
 *   wn_grad_norm_live          wn_grad_norm over the live elements: the same finalize launch, the same state block, the same
 *                              promises (grid a function of n_live alone, fixed order at every level, exact products in double:
 *                              non-finite exactly when a LIVE element is).  scratch: wn_grad_norm_scratch_floats(n) floats.
 *   wn_adam_step_live          wn_adam_step (ema == NULL) / wn_adam_step_ema: a live element's params, exp_avg, exp_avg_sq and
 *                              ema get the bits the whole-buffer call gives them on the same inputs and scalars.
 *   wn_adam_step_guarded_live  wn_adam_step_guarded (ema == NULL) / wn_adam_step_guarded_ema, likewise.
 * Errors (wn_last_error): a NULL buffer or table, n_ranges <= 0, n_live outside [n_ranges, n], and those of the calls above. */
int64_t wn_live_table(const int64_t* ranges, int n_ranges, int64_t n, int64_t* table);
int wn_grad_norm_live(const float* grads, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, float max_norm, int guard,
                      float lr, float beta1, float beta2, float* scratch, WnOptState* state, void* stream);
int wn_adam_step_live(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                      const int64_t* table, int n_ranges, int64_t n_live, int64_t step, float lr, float beta1, float beta2, float eps,
                      float weight_decay, double ema_decay, int ema_warmup, void* stream);
int wn_adam_step_guarded_live(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                              const int64_t* table, int n_ranges, int64_t n_live, float eps, float weight_decay,
                              const WnOptState* state, double ema_decay, int ema_warmup, void* stream);

/* ---- parameter groups: per-group lr, eps and weight decay in ONE Adam launch (since ABI v17; additions only) ----
 * Betas, the step count with its bias correction, the global gradient norm with its clip coefficient, the apply flag and the
 * moving average stay one per optimizer.  A group has four values: */
#define WN_MAX_PARAM_GROUPS 16
typedef struct WnAdamGroup {
    float lr;
    float eps;
    float weight_decay;
    int32_t decoupled; /* 0: L2 decay inside the gradient (torch.optim.Adam); != 0: decoupled decay (torch.optim.AdamW) */
} WnAdamGroup;
/* What the Adam launch reads per group, 16 bytes.  The unguarded call forms WN_MAX_PARAM_GROUPS of them on the host and passes them
 * as launch arguments; on the guarded path wn_grad_norm_groups writes them to a caller-owned device block of
 * WN_MAX_PARAM_GROUPS * sizeof(WnGroupScalars) = 256 bytes (4-byte aligned), which depends on nothing it held before. */
typedef struct WnGroupScalars {
    float lr_over_bc1; /* lr_g / (1 - beta1^step), formed in double (0 when the step does not apply) */
    float eps;
    float l2;          /* the coefficient of the L2 term: weight_decay_g, 0 for a decoupled group */
    float scale;       /* f_g = (float)(1.0 - (double)lr_g * (double)weight_decay_g) for a decoupled group, exactly 1 otherwise */
} WnGroupScalars;
/* For a live element i of group g at applied step t:
 *   L2 group         exactly the update of wn_adam_step* with lr_g / bc1, eps_g and weight_decay_g in the places of the global
 *                    scalars: params, exp_avg, exp_avg_sq and ema receive the bits the single-group entry point (wn_adam_step,
 *                    _ema, _guarded, _guarded_ema or their _live forms) gives that element for the same inputs, state block and
 *                    scalars.
 *   decoupled group  torch.optim.AdamW: p_d = p * f_g as one separately rounded product; the gradient gets no decay term (after
 *                    clipping it is clip_coef * g[i], as above); the moments as above; p_new = p_d - lr_g / bc1 * (m / denom).
 *                    With weight_decay_g == 0, f_g is exactly 1 and the element gets the bits of an L2 group with no decay.
 *
 * wn_group_table (host only, no launch): wn_live_table for triples lo, hi, group -- the ranges sorted, disjoint, non-empty and
 * inside [0, n), group in [0, n_groups).  It writes 4 * n_ranges int64 words to `table` (host memory): lo[n_ranges],
 * hi[n_ranges], before[n_ranges] -- exactly the words wn_live_table writes for the same ranges, so wn_grad_norm_live reads the
 * table as it is -- and group[n_ranges]; returns n_live, -1 on an error (wn_last_error: those of wn_live_table, a group index
 * outside [0, n_groups), n_groups outside [1, WN_MAX_PARAM_GROUPS]).  Frozen parameters compose: the ranges are the live ranges
 * split at group boundaries, and an element outside every range is neither read nor written in any buffer.  A group may own no
 * range.  The launching calls trust the device copy (8-byte aligned) to be what wn_group_table wrote.
 *
 *   wn_adam_step_groups          the unguarded step, ONE launch with the grid, the table cursor and the LDS staging of
 *                                wn_adam_step_live (the group block is staged beside the table; a thread picks up the four
 *                                scalars of a range when it enters it; a block walks a contiguous share of the compacted
 *                                space, so a table with a range per tensor costs no search per element).  The host forms lr_g / bc1, sqrt(bc2) and f_g in double as
 *                                wn_adam_step does; `groups` is host memory and travels in the launch arguments, so a learning rate
 *                                that changes every step costs no copy and no synchronisation.  ema == NULL: no moving average.
 *   wn_grad_norm_groups          two launches.  table == NULL: the sum of squares of wn_grad_norm over [0, n) without
 *                                [skip_lo, skip_hi) (a model with nothing frozen: the same launch, the same bits); otherwise that
 *                                of wn_grad_norm_live over the table (skip_lo == skip_hi == 0).  The finalize launch fills `state`
 *                                bit for bit as wn_grad_norm(_live) does with lr = groups[0].lr (WnOptState keeps its 56 bytes) and
 *                                writes all WN_MAX_PARAM_GROUPS entries of `group_scalars` (zeros behind n_groups), lr_g / bc1 by
 *                                the double formula of the state block from the device's count of applied steps.
 *   wn_adam_step_guarded_groups  wn_adam_step_guarded(_ema) over the table with the scalars of `group_scalars` and `state` as the
 *                                preceding wn_grad_norm_groups on the same stream left them; when apply == 0 nothing is written
 *                                in any group.
 * Errors (wn_last_error): those of the _live calls; groups or group_scalars NULL; n_groups outside [1, WN_MAX_PARAM_GROUPS];
 * group_scalars not 4-byte aligned; wn_grad_norm_groups with a table AND a skip range, or (table == NULL) a skip range outside
 * [0, n]. */
int64_t wn_group_table(const int64_t* triples, int n_ranges, int64_t n, int n_groups, int64_t* table);
int wn_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                        const int64_t* table, int n_ranges, int64_t n_live, int64_t step, const WnAdamGroup* groups, int n_groups,
                        float beta1, float beta2, double ema_decay, int ema_warmup, void* stream);
int wn_grad_norm_groups(const float* grads, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, int64_t skip_lo,
                        int64_t skip_hi, float max_norm, int guard, const WnAdamGroup* groups, int n_groups, float beta1,
                        float beta2, float* scratch, WnOptState* state, WnGroupScalars* group_scalars, void* stream);
int wn_adam_step_guarded_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                const int64_t* table, int n_ranges, int64_t n_live, const WnGroupScalars* group_scalars,
                                const WnOptState* state, double ema_decay, int ema_warmup, void* stream);

/* ---- layer-wise adaptive steps (LAMB) and per-tensor norms (since ABI v20; additions only) ----
 * A per-tensor trust ratio on top of the grouped Adam update (You et al. 2019), for batch sizes far above the one a recipe's
 * learning rate was tuned at.  For tensor k of group g at applied step t (1-based: `step` unguarded, the state block's
 * steps_applied guarded), bc1 = 1 - beta1^t and bc2 = 1 - beta2^t formed in double:
 *     ghat = clip_coef * grad                     (guarded; one separately rounded product, grad itself keeps its values)
 *     L2 group:        ghat += wd_g * p           (before the moments, as in wn_adam_step*)
 *     m, v             the expressions of wn_adam_step*: an adapted tensor's moments are the grouped launch's bit for bit
 *     u    = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps_g)
 *     decoupled group: u = fma(wd_g, p, u)
 *     wn_k = sqrt(sum p^2), un_k = sqrt(sum u^2)  over the tensor, p BEFORE the update, both sums in double
 *     r_k  = wn_k == 0 or un_k == 0 ? 1 : wn_k / un_k;   r_k = min(r_k, max_trust) when max_trust > 0
 *     p    = fma(-(lr_g * r_k), u, p);   ema = fmaf(w, p_new - ema, ema), w as in wn_adam_step_ema
 * A tensor that does not adapt takes the grouped Adam update: params, exp_avg, exp_avg_sq and ema receive the bits
 * wn_adam_step_groups / wn_adam_step_guarded_groups give them for the same inputs.  Guard: when apply == 0 nothing is written --
 * weights, moments, average and `stats` stay.  An element outside every range is neither read nor written in any buffer.
 * Guard off and a non-finite gradient: the norm of u is not finite, so the ratio and with it EVERY weight of that tensor is
 * poisoned (plain Adam poisons the one element); no other tensor is touched.  Use the guard.
 *
 * wn_tensor_table (host only, no launch): wn_group_table for quadruples lo, hi, group, adapt (0 | 1) -- ONE range per tensor, never
 * coalesced.  It writes at most 7 * n_ranges + 1 + n / WN_TENSOR_CHUNK int64 words (size `table` for that; copy them all to the
 * device): the four rows of wn_group_table (the _live and _groups norm calls read the table as it is), adapt[n_ranges],
 * block0[n_ranges] = the index of the first block of each range, the number of blocks, and the range of every block.
 * Every range owns ceil(len / WN_TENSOR_CHUNK) blocks of its own: the grid and every summation order are functions of the table
 * alone (and of the buffers' address modulo 16), never of the device, so data-parallel ranks derive the same ratios bit for bit
 * without communicating.  Returns n_live, -1 on an error (wn_last_error: those of wn_group_table, an adapt flag that is not 0 | 1).
 * wn_tensor_blocks: the number of blocks of a HOST table; wn_lamb_scratch_floats(n_blocks): floats of scratch (8-byte aligned)
 * wn_lamb_step and wn_tensor_sumsq need for it.
 *
 *   wn_lamb_step     three launches: (1) per block of an adapted range the moments, u and the sums of p^2 and u^2 in double, one
 *                    pair of partials per block, no atomics -- a range that does not adapt gets its whole Adam update here; (2)
 *                    per tensor the partials in block order -> stats[3 k .. 3 k + 2] = wn_k, un_k, r_k as floats (a tensor that
 *                    does not adapt: 0, 0, 1); (3) adapted ranges again: u recomputed from the stored moments, the weight and the
 *                    average written (10 words per element in all, no n-sized temporary).  16-byte accesses where the buffers
 *                    share their address modulo 16.  state == NULL: the unguarded step with `step`; otherwise `step` is ignored
 *                    and apply, clip_coef, steps_applied and the betas are read from `state` as the preceding wn_grad_norm* call
 *                    on the same stream left them (WnOptState keeps its 56 bytes).  `groups` is host memory and travels in the
 *                    launch arguments.  ema == NULL: no moving average.  max_trust == 0: no clamp.
 *   wn_tensor_sumsq  the same segmented reduction for any flat fp32 buffer of n elements: out[k] (device, double) = the sum of
 *                    x[i]^2 over range k.  Two launches.
 * Errors (wn_last_error): those of the _groups calls; max_trust < 0 or NaN; scratch, stats or out NULL; scratch / out not
 * 8-byte aligned. */
#define WN_TENSOR_CHUNK 8192
int64_t wn_tensor_table(const int64_t* quads, int n_ranges, int64_t n, int n_groups, int64_t* table);
int64_t wn_tensor_blocks(const int64_t* table, int n_ranges);
int64_t wn_lamb_scratch_floats(int64_t n_blocks);
int wn_tensor_sumsq(const float* x, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, float* scratch, double* out,
                    void* stream);
int wn_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, const int64_t* table,
                 int n_ranges, int64_t n_live, int64_t step, const WnAdamGroup* groups, int n_groups, float beta1, float beta2,
                 float max_trust, const WnOptState* state, double ema_decay, int ema_warmup, float* scratch, float* stats,
                 void* stream);

/* Low-rank adapters over the flat buffers (since ABI v22): W = W0 + scale B A for a table of matrices, as two fused operations.
 * An entry names a row-major [rows, cols] matrix W at w_off of the MODEL's flat buffers (a conv weight (out, in, K) is
 * [out, in K]) and its factors in the ADAPTER's flat buffer: A [rank, cols] at a_off, B [rows, rank] at b_off.  Offsets are in
 * elements and need no alignment beyond the element's; the kernels use 16-byte accesses on the runs of a row whose addresses allow
 * it, with a scalar head and tail.
 *
 * wn_lora_table (host only, no launch) checks the entries -- 1 <= rank <= WN_LORA_MAX_RANK, rank <= min(rows, cols), a finite
 * scale (as a float), every range inside its buffer (n_model / n_adapter elements), no two ranges overlapping in either buffer --
 * and lays out the blocks: 64 x 64 tiles of every matrix and chunks of 256 adapter-gradient elements, so the grids and every
 * summation order are functions of the entries alone, never of the device: data-parallel ranks derive the same bits.  Returns the
 * int64 words the table takes, and writes them when table != NULL and table_words is at least that (call it with NULL first);
 * -1 on an error.  The calls below take the host table AND a device copy of the same words.
 * wn_lora_scratch_floats(table): floats of scratch wn_lora_project needs for a HOST table; -1 when it is none.
 *
 *   wn_lora_merge    params[i] = fmaf(scale, acc, base[i]) with acc = 0, acc = fmaf(B[o,k], A[k,c], acc) for k = 0 .. rank - 1, on
 *                    every element of every entry: ONE launch.  base and params hold n_model elements and must not overlap;
 *                    an element outside every entry is neither read nor written in any buffer.
 *   wn_lora_project  adapter_grads: dA[k,c] = scale sum_o B[o,k] g[o,c] at a_off, dB[o,k] = scale sum_c g[o,c] A[k,c] at b_off,
 *                    g the entry's matrix in `grads`.  fp32 fma chains inside a tile (rows / columns ascending), the tiles'
 *                    shares added in tile order, one multiplication by scale; no atomics.  TWO launches: one over the tiles of
 *                    g -- each read from memory once -- that writes the shares into scratch, one that sums them.  grads and
 *                    adapter are only read; adapter_grads outside the ranges of A and B is not written.
 * Errors (wn_last_error): NULL or misaligned pointers (4 bytes; the tables 8), a table wn_lora_table did not write or that does
 * not fit n_model / n_adapter, scratch_floats below wn_lora_scratch_floats, base overlapping params, adapter overlapping
 * adapter_grads. */
#define WN_LORA_MAX_RANK 64
typedef struct WnLoraEntry {
    int64_t w_off, rows, cols, rank, a_off, b_off;
    double scale; /* alpha / rank; used as a float */
} WnLoraEntry;
int64_t wn_lora_table(const WnLoraEntry* entries, int n_entries, int64_t n_model, int64_t n_adapter, int64_t* table,
                      int64_t table_words);
int64_t wn_lora_scratch_floats(const int64_t* table);
int wn_lora_merge(const float* base, float* params, int64_t n_model, const float* adapter, int64_t n_adapter, const int64_t* table,
                  const int64_t* dev_table, void* stream);
int wn_lora_project(const float* grads, int64_t n_model, const float* adapter, float* adapter_grads, int64_t n_adapter,
                    const int64_t* table, const int64_t* dev_table, float* scratch, int64_t scratch_floats, void* stream);

/* ---- op-level entry points (used by the composite calls above; exported for parity tests) ---- */

/* a[i] <-> b[i] for i < n, in place and without a temporary buffer (since ABI v14): how the weights and their moving average change
 * places around a scoring pass.  Both pointers need 4-byte alignment only; pointers that share their address modulo 16 are moved
 * by 16-byte accesses with a scalar head and tail.  Bit patterns are moved as they are (NaN payloads included).  Overlapping
 * ranges are an error. */
int wn_op_swap(float* a, float* b, int64_t n, void* stream);

/* Gradient accumulation over micro-batches (since ABI v15): the sum of the gradients of several backward passes in front of
 * ONE optimizer step.  `acc` is the caller's accumulator, `grad` the gradient buffer wn_backward fills; both hold n floats.
 *     WN_ACCUM_SET     acc[i]  = grad[i]              first micro-batch: opens the sum, whatever acc held before
 *     WN_ACCUM_ADD     acc[i]  = acc[i] + grad[i]     a middle micro-batch
 *     WN_ACCUM_FINISH  grad[i] = acc[i] + grad[i]     last micro-batch: the sum lands in the gradient buffer itself, where
 *                                                     wn_grad_norm / wn_adam_step* and an all-reduce read it
 * One plain fp32 add per element, no scaling, no compensation: after SET, ADD, ..., FINISH over g0, g1, g2, ... the gradient
 * buffer holds ((g0 + g1) + g2) + ..., the bits of torch's `p.grad += g` in the same order.  NaN and +-inf propagate, so the
 * non-finite guard of wn_grad_norm sees a bad micro-batch in the sum.  The buffer a mode does not write is not written at all.
 * A pointer and a length: the call may cover a sub-range of the two flat buffers (a gradient bucket, wn_bucket_range), so both
 * pointers need 4-byte alignment only; pointers that share their address modulo 16 are moved by 16-byte accesses with a scalar
 * head and tail.  The grid depends on n alone.  One launch, 12 n bytes of traffic (8 n for WN_ACCUM_SET).
 * Errors (wn_last_error): NULL, n <= 0, a mode that is none of the three, overlapping ranges. */
enum { WN_ACCUM_SET = 0, WN_ACCUM_ADD = 1, WN_ACCUM_FINISH = 2 };
int wn_op_accumulate(float* acc, float* grad, int64_t n, int mode, void* stream);

/* OneHot + CausalConv1d(Q->R,K) as a gather (wavenet.py:78-92,513-516).  weight (R,Q,K), bias (R). */
int wn_op_front(const float* weight, const float* bias, const int64_t* x, float* out /*(B,R,T)*/, float* scratch /*K*Q*R*/,
                int B, int T, int Q, int R, int K, void* stream);

/* CausalConv1d forward (wavenet.py:95-121): y[b,:,t] = bias + sum_k W[:,:,k] x[b,:,t-(K-1-k)d].
 * weight (Cout,Cin,K) natural layout; scratch >= Cout*Cin*K floats. */
int wn_op_causal_conv(const float* weight, const float* bias, const float* x /*(B,Cin,T)*/, float* y /*(B,Cout,T)*/,
                      float* scratch, int B, int T, int Cin, int Cout, int K, int dilation, void* stream);

/* Backward of CausalConv1d (since ABI v9; the reference's module is an ordinary differentiable nn.Module, wavenet.py:95-121 --
 * autograd of Conv1d + slice): dx (B,Cin,T), dw (Cout,Cin,K), db (Cout) from dy (B,Cout,T); any of the three may be NULL.
 * Exact f32 matrix-core contractions, weight gradient as per-(sequence, time-chunk) partials summed in a fixed order.
 * scratch >= wn_op_causal_conv_backward_scratch_floats(B, T, Cin, Cout, K) floats. */
long wn_op_causal_conv_backward_scratch_floats(int B, int T, int Cin, int Cout, int K);
int wn_op_causal_conv_backward(const float* weight, const float* x, const float* dy, float* dx, float* dw, float* db,
                               float* scratch, int B, int T, int Cin, int Cout, int K, int dilation, void* stream);

/* UpSampling.forward (wavenet.py:124-154, since ABI v7): y (B, C, F*U) = x (B, C, F) through the (1, U) transposed
 * convolution with ONE kernel `weight` [U] and scalar `bias` (nullable) shared by all channels. */
int wn_op_upsampling(const float* weight, const float* bias, const float* x, float* y, int B, int C, int F, int U, void* stream);
/* dst (B, C, R) = src (B, R, C) with the last two axes swapped (LDS-tiled): the reference's logits are (B, T, n_quantize)
 * (wavenet.py:522), the kernels' (B, n_quantize, T) -- used for a gradient handed back by an external loss (train.py:534-538
 * through autograd).  src != dst. */
int wn_op_transpose_last2(const float* src, float* dst, int B, int R, int C, void* stream);

/* Generic C[z] = A.B contraction on the f32 matrix cores; argument block: wavenet_hip_gemm.h (struct WnGemmArgs,
 * the inline helper wn_gemm_default fills the neutral values). */
int wn_op_gemm(const struct WnGemmArgs* args, void* stream);

/* Mixture-of-logistics output head (BASELINE configs[3]).  NOT part of the reference (its WaveNet only has the
 * softmax head, wavenet.py:209-210,518-523): parity is therefore pinned to this repo's own CPU restatement of
 * the discretised mixture of logistics (PixelCNN++, Salimans et al. 2017) in oracle/, not to the reference.
 * out (B, out_channels = 3*n_mix, T) from wn_forward; y (B, T) fp32 target waveform in [-1, 1];
 * loss = mean negative log-likelihood over t >= t_start; dout goes to wn_backward as `dlogits`. */
int wn_mol_loss(const WnConfig* cfg, int B, int T, const float* out, const float* y, int t_start, float grad_scale,
                float loss_scale, int num_classes, float log_scale_min, float* loss, float* dout, void* workspace,
                size_t workspace_bytes, void* stream);

/* wn_mol_loss for a padded batch of unequal lengths (since ABI v11): t_end / n_loss, the mask and the divisor exactly as
 * wn_softmax_ce_loss_ragged defines them; y behind t_end[b] may hold anything finite, dout is exactly 0.0f there. */
int wn_mol_loss_ragged(const WnConfig* cfg, int B, int T, const float* out, const float* y, int t_start, const int32_t* t_end,
                       int64_t n_loss, float grad_scale, float loss_scale, int num_classes, float log_scale_min, float* loss,
                       float* dout, void* workspace, size_t workspace_bytes, void* stream);

/* ---- autoregressive decode (BASELINE config 5) -------------------------------------------------
 * Replaces WaveNet.fast_generate / batch_fast_generate / _generate_residual_forward
 * (wavenet_vocoder/nets/wavenet.py:309-395, 397-511, 538-549): one persistent workgroup per
 * utterance, the dilation queues in a caller-owned state buffer, tokens chosen on-chip.
 *
 * Positions index the left-padded token buffer `samples` (B, Ttot) (wavenet.py:331-336: the
 * context is padded with n_quantize/2 up to the receptive field, the aux features by replicating
 * their first column: pass the pad length as n_pad).  Step p reads the tokens at p-K+1..p and the
 * aux column of position p and produces the logits of position p+1.  Positions below t_forced[b]
 * are the context (teacher forced; running them from step 0 over a zeroed state IS the reference's
 * "prepare buffer" pass, wavenet.py:338-349); from t_forced[b] on, step p writes samples[b][p+1].
 * Utterance b stops at t_end[b] positions.  All pointers are device pointers; nothing is allocated;
 * asynchronous on `stream`.  The compiled kernel classes cover n_resch <= 64, n_skipch <= 256,
 * n_quantize <= 256, kernel_size <= 3: wn_decode_supported() tells, everything else returns an
 * error (callers fall back to full-window forwards, wavenet.py:243-307). */
int wn_decode_supported(const WnConfig* cfg);
int64_t wn_decode_pack_floats(const WnConfig* cfg);   /* floats of the packed decode weights, <0: unsupported */
int64_t wn_decode_state_floats(const WnConfig* cfg);  /* floats of queue state per utterance */
int64_t wn_decode_stream_bytes(const WnConfig* cfg);  /* weight bytes one workgroup streams per step */
/* Re-pack the flat parameter buffer into the per-thread weight stream + side tables. */
int wn_decode_pack(const WnConfig* cfg, const float* params, float* wpack, void* stream);
/* Aux projections of all layers at the aux rate: G[b][f][l*2R+o'] = Waux_l h[b][:, f] (wavenet.py:541-542).
 * h is (B, n_aux, F): frames if upsampling_factor > 0 (the kernel applies the transposed-conv taps
 * of wavenet.py:136 per sample), samples otherwise. */
int wn_decode_aux(const WnConfig* cfg, int B, int F, const float* wpack, const float* h, float* G, void* stream);
/* mode: 0 argmax, 1 categorical sampling with the caller's uniform draws `uniforms` (B, Ttot)
 * (draw [b][p+1] picks the token of position p+1), 2 mixture-of-logistics head (out_channels = 3*n_mix, n_mix <= 64;
 * not in the reference): uniforms is (B, Ttot, n_mix+1), the drawn value goes to wave_out (B, Ttot) (nullable) and,
 * mu-law encoded with n_quantize levels, to samples.  logits_out (B, Ttot, out_channels) is optional (row p = the
 * network output computed by step p).  `state` (B, wn_decode_state_floats) must be zero before step 0. */
int wn_decode_steps(const WnConfig* cfg, int B, const float* params, const float* wpack, const float* G, int F, int n_pad,
                    int64_t* samples, int64_t Ttot, const int32_t* t_forced, const int32_t* t_end, int p0, int p1,
                    float* state, const float* uniforms, float* logits_out, int mode, float* wave_out, float log_scale_min,
                    void* stream);

/* Any-size variant of the same decode (layer-wise launches of the contraction kernels on [channels x B]
 * operands: one pass over the weights per step serves the whole batch).  Same positions / teacher forcing
 * / mode / uniforms / logits_out conventions as wn_decode_steps.  `state` is ONE caller-owned buffer of
 * wn_decode_layered_state_floats(cfg, B, mode) floats, zero-filled before wn_decode_layered_prepare, which packs
 * the weights into it and computes G (B, F, L*2R) from h (B, n_aux, F).  A later wn_decode_layered_prepare on the
 * same state with params == NULL keeps the packed weights and only projects the given window of h (a decode
 * without an upsampling layer projects one window of aux columns per chunk of steps). */
int64_t wn_decode_layered_state_floats(const WnConfig* cfg, int B, int mode);
/* Since ABI v7: for models the plan of csrc/wn_dlp.h covers (n_resch % 32 == 0, kernel_size 2 or 3, B <= 64 (48 with the granule hand-off), softmax head)
 * wn_decode_layered_steps runs the whole range of steps as ONE launch of workgroups that hand their vectors to each other as
 * 8-byte {value, tag} granules or as plain vectors + one flag per workgroup and stage (the recipes' n_resch = 512 model: 66
 * dependent launches per step before): n_resch / 4 workgroups with fp32 VALU dot products for one utterance (wn_dlp.hip),
 * n_resch / 8 workgroups per block of 16 utterances with v_mfma_f32_16x16x4_f32 tiles up to 64 (wn_dlpf.hip; wn_dlpm.hip: 48).
 * Every workgroup of such a launch waits for the others, so ALL of them must be resident at once: the library asks the device
 * (occupancy of the chosen kernel x compute units, since ABI v8) when it chooses the path, and a grid that does not fit -- a
 * partitioned GPU, a part with fewer CUs -- decodes by layer-wise launches; wn_decode_layered_residency() reports the numbers.
 * Mode bits (the SAME bits go to every call of one decode -- state_floats / error_offset / prepare / steps, and OR-ed into
 * `layered` of wn_decode_prefill -- because the layout of `state` depends on them):
 *   WN_DECODE_BY_LAUNCHES  wn_decode_layered_steps keeps the layer-wise launches (independent check, A/B, fall-back);
 *   WN_DECODE_GRANULES     (since ABI v8; replaces the process-wide wn_decode_set_handoff of v7) the persistent launches hand
 *                          their vectors over as 8-byte granules everywhere instead of plain vectors + one flag per workgroup
 *                          and stage where wn_dlpf.hip covers the plan (A/B, tests).
 * The persistent launch bounds every wait; wn_decode_layered_error_offset() is the float offset in `state` of an int that is
 * non-zero afterwards if a wait timed out (-1: this model / B / device decodes by launches).  A launch that finds the word
 * non-zero returns at once, so a caller may check it after any chunk of steps. */
#define WN_DECODE_BY_LAUNCHES 256
#define WN_DECODE_GRANULES 512
int64_t wn_decode_layered_error_offset(const WnConfig* cfg, int B, int mode);
/* 1: wn_decode_layered_steps(cfg, B, mode) runs as one persistent launch on the current device, 0: as layer-wise launches;
 * *workgroups (nullable) = the grid the plan asks for (0: no plan covers this model / B), *capacity (nullable) = workgroups of
 * that kernel the device keeps resident at once.  < 0: bad argument. */
int wn_decode_layered_residency(const WnConfig* cfg, int B, int mode, int* workgroups, int* capacity);
int wn_decode_layered_prepare(const WnConfig* cfg, int B, int F, const float* params, const float* h, float* G, float* state,
                              int64_t state_floats, int mode, void* stream);
int wn_decode_layered_steps(const WnConfig* cfg, int B, const float* params, const float* G, int F, int n_pad,
                            int64_t* samples, int64_t Ttot, const int32_t* t_forced, const int32_t* t_end, int p0, int p1,
                            float* state, int64_t state_floats, const float* uniforms, float* logits_out, int mode,
                            float* wave_out, float log_scale_min, void* stream);
/* mode 2 (mixture-of-logistics head, out_channels = 3*n_mix): uniforms is (B, Ttot, n_mix+1); the drawn value is
 * written to wave_out (B, Ttot) (nullable) and, mu-law encoded with n_quantize levels, to samples.  log_scale_min
 * (since ABI v4; ignored by modes 0/1) is the clamp of the log-scales -- pass the value the model was trained with
 * (wn_mol_loss's log_scale_min) so that sampling and the likelihood agree. */

/* Since ABI v21: temperature, top-k and nucleus (top-p) sampling -- the setting of one decode call, applied to mode 1 (sampling
 * on the softmax head) inside the decode kernels (csrc/wn_sample.h; up to 512 classes), in this order:
 *   1. s_q = fp32(logit_q * inv_temperature)      inv_temperature = (float)(1.0 / T), formed by the caller in double
 *   2. top_k > 0: v_k = the k-th largest s counted with multiplicity, A = {q : s_q >= v_k} (ties at v_k are all kept);
 *      top_k == 0 or >= the number of classes: off
 *   3. top_p < 1: with e_q = expf(s_q - s_max), tau = the largest v among {s_q : q in A} for which
 *      sum_{q in A, s_q >= v} e_q >= top_p * sum_{q in A} e_q, B = {q in A : s_q >= tau} (ties kept; the maximal class is in B)
 *   4. the draw of mode 1 restricted to B: in index order the first q in B whose running sum of e_q reaches u * total.
 * logits_out keeps receiving the raw logits.  The *_filtered calls take the arguments of their plain counterparts plus the
 * setting: NULL or the identity {1, 0, 1} IS the plain call (same launches, same tokens); a setting that is not the identity
 * together with mode 0 or 2 is an error, so is inv_temperature <= 0 or non-finite, top_k < 0, top_p outside (0, 1]. */
typedef struct WnSampling {
    float inv_temperature;
    int32_t top_k;
    float top_p;
} WnSampling;
int wn_decode_steps_filtered(const WnConfig* cfg, int B, const float* params, const float* wpack, const float* G, int F, int n_pad,
                             int64_t* samples, int64_t Ttot, const int32_t* t_forced, const int32_t* t_end, int p0, int p1,
                             float* state, const float* uniforms, float* logits_out, int mode, float* wave_out,
                             float log_scale_min, const WnSampling* sampling, void* stream);
int wn_decode_layered_steps_filtered(const WnConfig* cfg, int B, const float* params, const float* G, int F, int n_pad,
                                     int64_t* samples, int64_t Ttot, const int32_t* t_forced, const int32_t* t_end, int p0,
                                     int p1, float* state, int64_t state_floats, const float* uniforms, float* logits_out,
                                     int mode, float* wave_out, float log_scale_min, const WnSampling* sampling, void* stream);

/* Parallel context walk.  The reference builds the generation buffers with ONE full forward over the padded
 * context (wavenet.py:338-349, 427-441); stepping the decode kernel through those >= receptive-field positions
 * instead costs rf steps before the first new sample.  These three entry points do what the reference does:
 *   wn_decode_ctx_aux   h (B, n_aux, F) -> h_ctx (B, n_aux, Tctx): the UPSAMPLED aux feature of every context
 *                       position (ConvTranspose2d of wavenet.py:141-154), the n_pad left-padding positions
 *                       replicating the first upsampled column (wavenet.py:336, 425);
 *   wn_decode_prefill   runs the residual stack of the training forward on x_ctx (B, Tctx) / h_ctx and copies
 *                       the newest (K-1)*d_l layer inputs of every layer into the dilation queues of `state`
 *                       (layered = 0: the (B, wn_decode_state_floats) state of wn_decode_steps; 1 [| WN_DECODE_GRANULES
 *                       when the decode runs with that bit]: the state of wn_decode_layered_steps, after
 *                       wn_decode_layered_prepare).  The B utterances of the call
 *                       are utterances [state_b0, state_b0 + B) of a state built for state_B utterances, so a
 *                       large batch can be walked in groups with a bounded workspace.  Decoding then resumes
 *                       with p0 = Tctx-1, the last context position, whose logits choose the first new sample.
 *                       `ws`: wn_decode_prefill_workspace_bytes(cfg, B, Tctx) bytes; flags as wn_forward.
 * Tctx >= receptive field (the caller pads: wavenet.py:328-336).  Only the newest receptive field + kernel_size - 1
 * positions of a context reach the queues (the dilated stack plus the causal front conv), so a long context may be
 * passed as its tail of at least that many positions: x_ctx / h_ctx then hold positions [pos0, pos0 + Tctx) of
 * the padded context and decoding resumes with p0 = pos0 + Tctx - 1. */
int wn_decode_ctx_aux(const WnConfig* cfg, int B, int F, int Tctx, int n_pad, int pos0, const float* params, const float* h,
                      float* h_ctx, void* stream);
size_t wn_decode_prefill_workspace_bytes(const WnConfig* cfg, int B, int Tctx);
int wn_decode_prefill(const WnConfig* cfg, int B, int Tctx, int pos0, const float* params, const int64_t* x_ctx,
                      const float* h_ctx,
                      void* ws, size_t ws_bytes, float* state, int64_t state_floats, int state_B, int state_b0, int layered,
                      int flags, void* stream);

/* ---- diagnostics: opt-in per-launch timing with HIP events (used by bench.py's roofline block) ----
 * wn_prof_enable(1) clears and starts recording {kernel tag, algorithmic flops/bytes, start/stop
 * event} for every launch; after synchronising, wn_prof_report writes a JSON object
 * {"tag": {"count", "ms", "flops", "bytes"}} into buf (returns the needed size when buf == NULL). */
int wn_prof_enable(int on);
int wn_prof_report(char* buf, size_t n);
/* the recorded tags in issue order, comma separated; "bucket_event" marks where wn_backward recorded a gradient-bucket
 * event (tests assert that a bucket's event follows the last launch that writes into the bucket).  Same buffer protocol. */
int wn_prof_sequence(char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* WAVENET_HIP_H_ */
