// wn_optim.h -- launchers of the optimizer-side kernels (wn_optim.inl): Adam over a flat fp32 buffer in its four variants, the
// global gradient norm, the in-place exchange of two buffers and gradient accumulation.  They depend on nothing of the network:
// struct WnOptState, the group structs and WN_ACCUM_* (include/wavenet_hip.h) are all they share with the rest of the library.
#pragma once
#include "wn_device.h"

#include "../../include/wavenet_hip.h"   // struct WnAdamGroup, struct WnGroupScalars, WN_MAX_PARAM_GROUPS

// Adam over a flat fp32 buffer (torch.optim.Adam semantics, train.py:457-460): elements in
// [skip_lo, skip_hi) are left untouched (parameters that never receive a gradient).
int wn_adam(float* p, const float* g, float* m, float* v, long n, float lr_over_bc1, float inv_sqrt_bc2,
            float beta1, float beta2, float eps, float weight_decay, long skip_lo, long skip_hi, wn_stream_t st);

// Global gradient norm for clipping / the non-finite-step guard (struct WnOptState: include/wavenet_hip.h).
//   wn_grad_sumsq:         partial[b] = sum of g[i]^2 in double over block b's share of [0, n) minus [skip_lo, skip_hi);
//                          wn_grad_sumsq_blocks(n) partials, a function of n alone (never of the device)
//   wn_grad_norm_finalize: the partials in a fixed order -> norm, clip coefficient, apply flag, step counters and this step's
//                          lr / bc1, sqrt(bc2) in the state block
//   wn_adam_guarded:       wn_adam with those scalars read from the state block; writes nothing when the step does not apply
struct WnOptState;
int wn_grad_sumsq_blocks(long n);
int wn_grad_sumsq(const float* g, long n, long skip_lo, long skip_hi, double* partial, wn_stream_t st);
int wn_grad_norm_finalize(const double* partial, int nb, float max_norm, int guard, float lr, float beta1, float beta2,
                          struct WnOptState* state, wn_stream_t st);
int wn_adam_guarded(float* p, const float* g, float* m, float* v, long n, float eps, float weight_decay, long skip_lo, long skip_hi,
                    const struct WnOptState* state, wn_stream_t st);

// Exponential moving average of the weights inside the Adam launch (include/wavenet_hip.h, ABI v14): e += w (p_new - e).
// wn_ema_weight is the ONE place the averaging weight w = (float)(1 - d_t) is formed, in double, for the host (unguarded step: t =
// the caller's step) and for every thread of the guarded launch (t = the state block's steps_applied): the same t gives the same
// bits.  d_t = min(decay, (1 + t) / (10 + t)) with the warm-up, else decay; t counts the applied steps from 1.
static __host__ __device__ __forceinline__ float wn_ema_weight(double decay, int warmup, int64_t t) {
    double d = decay;
    if (warmup) {
        const double dw = (1.0 + (double)t) / (10.0 + (double)t);
        if (dw < d) d = dw;
    }
    return (float)(1.0 - d);
}
int wn_adam_ema(float* p, const float* g, float* m, float* v, float* e, long n, float lr_over_bc1, float sqrt_bc2, float beta1,
                float beta2, float eps, float weight_decay, long skip_lo, long skip_hi, float w, wn_stream_t st);
int wn_adam_guarded_ema(float* p, const float* g, float* m, float* v, float* e, long n, float eps, float weight_decay, long skip_lo,
                        long skip_hi, const struct WnOptState* state, double ema_decay, int ema_warmup, wn_stream_t st);
// The same over LIVE RANGES of the buffers (training with frozen parameters; include/wavenet_hip.h, ABI v16).  `table` is the
// device table wn_live_table wrote (lo[nr], hi[nr], before[nr]), n_live its number of live elements.  The kernels walk the
// compacted index space [0, n_live) with the grid of the whole-buffer launch for n_live elements and address nothing outside the
// ranges; a live element gets the bits the whole-buffer launch gives it.  e == NULL: no moving average.
int wn_adam_live(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, float lr_over_bc1,
                 float sqrt_bc2, float beta1, float beta2, float eps, float weight_decay, float w, wn_stream_t st);
int wn_adam_guarded_live(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, float eps,
                         float weight_decay, const struct WnOptState* state, double ema_decay, int ema_warmup, wn_stream_t st);
// wn_grad_sumsq_blocks(n_live) partials for wn_grad_norm_finalize
int wn_grad_sumsq_live(const float* g, const long* table, int nr, long n_live, double* partial, wn_stream_t st);
// The Adam launches over PARAMETER GROUPS (include/wavenet_hip.h, ABI v17): `table` is the device copy of what wn_group_table wrote
// (lo[nr], hi[nr], before[nr], group[nr]), the grid and the walk are those of wn_adam_live, and every range is updated with the
// four scalars of its group.  wn_adam_groups takes the group block from the host (`block`: WN_MAX_PARAM_GROUPS entries, passed
// on as a launch argument), wn_adam_guarded_groups reads the device block wn_grad_norm_finalize_groups left behind the state
// block it fills exactly as wn_grad_norm_finalize does with lr = groups[0].lr.  e == NULL: no moving average.
// The ONE place a group's four scalars are formed, in double, for the host (unguarded step: bc1 from the caller's step) and for
// the finalize launch (guarded: bc1 from the device's count): the same inputs give the same bits on both paths.
static __host__ __device__ __forceinline__ WnGroupScalars wn_group_scalars(const WnAdamGroup& a, double bc1, bool apply) {
    WnGroupScalars s;
    s.lr_over_bc1 = apply ? (float)((double)a.lr / bc1) : 0.0f;
    s.eps = a.eps;
    s.l2 = a.decoupled ? 0.0f : a.weight_decay;
    s.scale = a.decoupled ? (float)(1.0 - (double)a.lr * (double)a.weight_decay) : 1.0f;
    return s;
}

int wn_adam_groups(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                   const struct WnGroupScalars* block, float sqrt_bc2, float beta1, float beta2, float w, wn_stream_t st);
int wn_adam_guarded_groups(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                           const struct WnGroupScalars* dev_block, const struct WnOptState* state, double ema_decay, int ema_warmup,
                           wn_stream_t st);
int wn_grad_norm_finalize_groups(const double* partial, int nb, float max_norm, int guard, const struct WnAdamGroup* groups,
                                 int n_groups, float beta1, float beta2, struct WnOptState* state, struct WnGroupScalars* block,
                                 wn_stream_t st);
// Layer-wise adaptive steps and per-tensor sums of squares over a TENSOR table (include/wavenet_hip.h, ABI v20; wn_tensor_table
// wrote it).  wn_bias_correction is the ONE place the two bias corrections of an applied step t are formed, in double, for the host
// (unguarded step: t = the caller's step) and for every thread of the guarded launches (t = the state block's steps_applied).
struct WnBiasCorrection {
    double bc1, bc2;
};
static __host__ __device__ __forceinline__ WnBiasCorrection wn_bias_correction(float beta1, float beta2, int64_t t) {
    return {1.0 - pow((double)beta1, (double)t), 1.0 - pow((double)beta2, (double)t)};
}
// three launches (moments + partial sums, ratios, apply); state == NULL: the unguarded step with the host's `step`, otherwise
// apply, clip_coef, steps_applied and the betas come from the state block.  partial: 2 doubles per block; stats: 3 floats per range
int wn_lamb(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, long step,
            const struct WnAdamGroup* groups, int n_groups, float beta1, float beta2, float max_trust, const struct WnOptState* state,
            double ema_decay, int ema_warmup, double* partial, float* stats, wn_stream_t st);
// out[r] = sum of x[i]^2 over range r of the table, in double (two launches; partial: one double per block)
int wn_tensor_sumsq_launch(const float* x, const long* table, int nr, long n_live, double* partial, double* out, wn_stream_t st);
// a[i] <-> b[i], i < n: two non-overlapping fp32 buffers of 4-byte alignment, exchanged in place
int wn_swap(float* a, float* b, long n, wn_stream_t st);
// gradient accumulation over micro-batches (include/wavenet_hip.h WN_ACCUM_*, ABI v15): SET acc = grad, ADD acc = acc + grad,
// FINISH grad = acc + grad; two non-overlapping fp32 buffers of 4-byte alignment, one plain fp32 add per element
int wn_grad_accumulate(float* acc, float* grad, long n, int mode, wn_stream_t st);
