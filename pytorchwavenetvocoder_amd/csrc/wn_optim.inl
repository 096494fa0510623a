// wn_optim.inl -- the optimizer side of the training step (gfx950): Adam over one flat fp32 buffer, the global gradient norm
// behind clipping and the non-finite-step guard, the in-place exchange of two buffers and gradient accumulation.  All of it is
// HBM-bound streaming over flat buffers; nothing here knows the network (struct WnOptState and WN_ACCUM_* are the whole interface).
// Part of wn_elem.hip (included at its end, like wn_auxdh.inl; WN_TPB is that file's).  Not compiled on its own.
#include "wn_optim.h"

#include "../../include/wavenet_hip.h"   // struct WnOptState, WN_ACCUM_*

// ---------------------------------------------------------------------------------------------
// Buffers here are 4-byte aligned only (a view, a bucket range, starts at any float offset).  A kernel that wants 16-byte accesses
// walks `n4` quads behind `head` scalar elements in front of the first 16-byte boundary; the up to 3 + 3 scalar elements of head
// and tail go to threads 0..3 and 4..7 of block 0.
struct WnQuadSplit {
    long head, n4;
};
static __device__ __forceinline__ WnQuadSplit wn_quad_split(const float* p, long n) {
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
    if (head > n) head = n;
    return {head, (n - head) >> 2};
}
// true for the threads that own a scalar head or tail element, *i = its index
static __device__ __forceinline__ bool wn_quad_edge(const WnQuadSplit& s, long n, long* i) {
    if (blockIdx.x != 0 || threadIdx.x >= 8) return false;
    const long t = threadIdx.x & 3;
    *i = threadIdx.x < 4 ? t : s.head + 4 * s.n4 + t;
    return *i < (threadIdx.x < 4 ? s.head : n);
}
// one thread per quad, at most `cap` blocks: a function of n alone (never of the device)
static unsigned wn_quad_blocks(long n, long cap) {
    const long nb = ((n + 3) / 4 + WN_TPB - 1) / WN_TPB;
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

// ---------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam semantics) in its four variants, the update written ONCE:
//   GUARDED  the scalars come from the state block wn_grad_norm_finalize left; the gradient is scaled by clip_coef
//            BEFORE the weight-decay term (torch clips the raw gradient, the optimizer adds L2 decay afterwards), g itself is left
//            as it is, and a step that does not apply writes nothing (the kernels return before the sweep)
//   EMA      with the new weight still in a register, e += w (p_new - e) as ONE fma.  The increment form has
//            e == p_new as its exact fixed point; d e + (1 - d) p_new has not (the two fp32 coefficients of d = 0.9999 do not sum
//            to 1).  9 words per element move instead of 7.
// Both are compile-time: a plain kernel carries no multiply by a coefficient and no access to e.  p, m and v get the same bits
// from all four kernels because there is one expression for them (wn_adam_element), which no flag changes: GUARDED only puts a
// separately rounded product in place of g[i], and the EMA only reads pn.  The kernels over live ranges (below) call the same one.
//   SCALE    (the kernels over parameter groups only) the weight enters as the separately rounded product
//            pscale * p[i]: torch.optim.AdamW's decoupled decay, p *= 1 - lr wd, in front of an update whose gradient carries no
//            decay term (such a group passes wd = 0).  An L2 group passes pscale = 1, which is exact: the arithmetic below is the
//            one of SCALE = false, which no other kernel leaves.
// the two moments from the values of one element (pv: the weight as the L2 term sees it); the layer-wise kernels (below) form
// theirs with this very expression, so an adapted tensor's moments are the grouped launch's bit for bit
template <bool GUARDED>
static __device__ __forceinline__ void wn_adam_moments(float pv, float g, float m, float v, float coef, float beta1, float beta2,
                                                       float wd, float* m_new, float* v_new) {
    // never contracted into the decay term's fma: coef == 1 leaves the unguarded arithmetic
    float gv = GUARDED ? wn_fmul_rn(coef, g) : g;
    // gv += wd * pv;  m = beta1 * m + (1 - beta1) * gv;  v = beta2 * v + (1 - beta2) * gv * gv -- with the products hipcc has
    // always fused here named, so that a kernel with another loop shape (16-byte quads) cannot fuse the other ones
    if (wd != 0.0f) gv = wn_fma_contracted(wd, pv, gv);
    *m_new = wn_fma_contracted(beta1, m, wn_fmul_rn(1.0f - beta1, gv));
    *v_new = wn_fma_contracted(beta2, v, wn_fmul_rn(wn_fmul_rn(1.0f - beta2, gv), gv));
}

template <bool GUARDED, bool EMA, bool SCALE = false>
static __device__ __forceinline__ void wn_adam_element(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ e, long i, float lr_over_bc1,
                                                       float sqrt_bc2, float coef, float beta1, float beta2, float eps, float wd,
                                                       float w, float pscale = 1.0f) {
    const float pv = SCALE ? wn_fmul_rn(pscale, p[i]) : p[i];
    float ev = 0.0f;
    if (EMA) ev = e[i];
    float mv, vv;
    wn_adam_moments<GUARDED>(pv, g[i], m[i], v[i], coef, beta1, beta2, wd, &mv, &vv);
    m[i] = mv;
    v[i] = vv;
    const float denom = sqrtf(vv) / sqrt_bc2 + eps;
    const float pn = pv - lr_over_bc1 * (mv / denom);
    p[i] = pn;
    if (EMA) e[i] = fmaf(w, pn - ev, ev);
}

// the whole buffer without [skip_lo, skip_hi): one element per thread and trip
template <bool GUARDED, bool EMA>
static __device__ __forceinline__ void wn_adam_sweep(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, float* __restrict__ e, long n, float lr_over_bc1,
                                                     float sqrt_bc2, float coef, float beta1, float beta2, float eps, float wd,
                                                     long skip_lo, long skip_hi, float w) {
    const long stride = (long)gridDim.x * WN_TPB;
    for (long i = (long)blockIdx.x * WN_TPB + threadIdx.x; i < n; i += stride) {
        if (i >= skip_lo && i < skip_hi) continue;
        wn_adam_element<GUARDED, EMA>(p, g, m, v, e, i, lr_over_bc1, sqrt_bc2, coef, beta1, beta2, eps, wd, w);
    }
}

__global__ __launch_bounds__(WN_TPB) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, long n, float lr_over_bc1, float sqrt_bc2, float beta1,
                                                 float beta2, float eps, float wd, long skip_lo, long skip_hi) {
    wn_adam_sweep<false, false>(p, g, m, v, nullptr, n, lr_over_bc1, sqrt_bc2, 1.0f, beta1, beta2, eps, wd, skip_lo, skip_hi, 0.0f);
}

__global__ __launch_bounds__(WN_TPB) void k_adam_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, long n, float eps, float wd, long skip_lo,
                                                         long skip_hi, const WnOptState* __restrict__ state) {
    if (!state->apply) return;
    wn_adam_sweep<true, false>(p, g, m, v, nullptr, n, state->lr_over_bc1, state->sqrt_bc2, state->clip_coef, state->beta1,
                               state->beta2, eps, wd, skip_lo, skip_hi, 0.0f);
}

__global__ __launch_bounds__(WN_TPB) void k_adam_ema(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ v, float* __restrict__ e, long n, float lr_over_bc1,
                                                     float sqrt_bc2, float beta1, float beta2, float eps, float wd, long skip_lo,
                                                     long skip_hi, float w) {
    wn_adam_sweep<false, true>(p, g, m, v, e, n, lr_over_bc1, sqrt_bc2, 1.0f, beta1, beta2, eps, wd, skip_lo, skip_hi, w);
}

// the averaging weight from the device's own count of applied steps (this one included: the finalize launch has counted it)
__global__ __launch_bounds__(WN_TPB) void k_adam_guarded_ema(float* __restrict__ p, const float* __restrict__ g,
                                                             float* __restrict__ m, float* __restrict__ v, float* __restrict__ e,
                                                             long n, float eps, float wd, long skip_lo, long skip_hi,
                                                             const WnOptState* __restrict__ state, double ema_decay,
                                                             int ema_warmup) {
    if (!state->apply) return;
    const float w = wn_ema_weight(ema_decay, ema_warmup, state->steps_applied);
    wn_adam_sweep<true, true>(p, g, m, v, e, n, state->lr_over_bc1, state->sqrt_bc2, state->clip_coef, state->beta1, state->beta2,
                              eps, wd, skip_lo, skip_hi, w);
}

static unsigned wn_adam_blocks(long n) {
    long nb = (n + WN_TPB - 1) / WN_TPB;
    return (unsigned)(nb > 2048 ? 2048 : (nb < 1 ? 1 : nb));
}

int wn_adam(float* p, const float* g, float* m, float* v, long n, float lr_over_bc1, float sqrt_bc2, float beta1, float beta2,
            float eps, float weight_decay, long skip_lo, long skip_hi, wn_stream_t st) {
    WN_PROF("adam", 0.0, 0.0, st);
    WN_LAUNCH(k_adam, dim3(wn_adam_blocks(n)), dim3(WN_TPB), 0, st, p, g, m, v, n, lr_over_bc1, sqrt_bc2, beta1, beta2, eps,
              weight_decay, skip_lo, skip_hi);
    return 0;
}

int wn_adam_guarded(float* p, const float* g, float* m, float* v, long n, float eps, float weight_decay, long skip_lo, long skip_hi,
                    const WnOptState* state, wn_stream_t st) {
    WN_PROF("adam_guarded", 0.0, 0.0, st);
    WN_LAUNCH(k_adam_guarded, dim3(wn_adam_blocks(n)), dim3(WN_TPB), 0, st, p, g, m, v, n, eps, weight_decay, skip_lo, skip_hi,
              state);
    return 0;
}

int wn_adam_ema(float* p, const float* g, float* m, float* v, float* e, long n, float lr_over_bc1, float sqrt_bc2, float beta1,
                float beta2, float eps, float weight_decay, long skip_lo, long skip_hi, float w, wn_stream_t st) {
    WN_PROF("adam_ema", 0.0, 36.0 * (double)n, st);
    WN_LAUNCH(k_adam_ema, dim3(wn_adam_blocks(n)), dim3(WN_TPB), 0, st, p, g, m, v, e, n, lr_over_bc1, sqrt_bc2, beta1, beta2, eps,
              weight_decay, skip_lo, skip_hi, w);
    return 0;
}

int wn_adam_guarded_ema(float* p, const float* g, float* m, float* v, float* e, long n, float eps, float weight_decay, long skip_lo,
                        long skip_hi, const WnOptState* state, double ema_decay, int ema_warmup, wn_stream_t st) {
    WN_PROF("adam_guarded_ema", 0.0, 36.0 * (double)n, st);
    WN_LAUNCH(k_adam_guarded_ema, dim3(wn_adam_blocks(n)), dim3(WN_TPB), 0, st, p, g, m, v, e, n, eps, weight_decay, skip_lo, skip_hi,
              state, ema_decay, ema_warmup);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Global-norm clipping and the non-finite-step guard (wn_grad_norm / wn_adam_step_guarded).
// k_grad_sumsq: one double per block = sum of g[i]^2 over the block's share of [0, n) minus [skip_lo, skip_hi).  Every product
// (double)g * (double)g is exact (48 significand bits) and no sum of n such squares can leave double's range, so the total is
// non-finite exactly when an element outside the skip range is.  The grid (wn_grad_sumsq_blocks) depends on n alone and every
// level of the sum -- per thread front to back, the xor butterfly of a wave, the waves of a block in order, the blocks in the
// finalize launch -- is a fixed order: the same buffer at the same address modulo 16 gives the same bits on every device.
#define WN_GN_MAXBLOCKS 512
#define WN_GN_BATCH 4
int wn_grad_sumsq_blocks(long n) { return (int)wn_quad_blocks(n, WN_GN_MAXBLOCKS); }

__global__ __launch_bounds__(WN_TPB) void k_grad_sumsq(const float* __restrict__ g, long n, long skip_lo, long skip_hi,
                                                       double* __restrict__ partial) {
    __shared__ double red[WN_TPB >> 6];
    const WnQuadSplit qs = wn_quad_split(g, n);
    const long head = qs.head, n4 = qs.n4;
    const float4* q = reinterpret_cast<const float4*>(g + head);
    const long stride = (long)gridDim.x * WN_TPB;
    double acc = 0.0;
    // WN_GN_BATCH quads per thread and trip, their 16-byte loads issued back to back (32 KiB in flight per CU at 8 waves per CU) and
    // no early exit in the body: a quad beyond the end re-reads quad j and adds zeros, an element inside the skip range adds
    // zero whatever it holds.  A thread still adds its quads j, j + stride, j + 2 stride, ... front to back.
    for (long j = (long)blockIdx.x * WN_TPB + threadIdx.x; j < n4; j += WN_GN_BATCH * stride) {
        float4 v[WN_GN_BATCH];
        WN_UNROLL
        for (int k = 0; k < WN_GN_BATCH; ++k) {
            const long jk = j + k * stride;
            v[k] = q[jk < n4 ? jk : j];
        }
        WN_UNROLL
        for (int k = 0; k < WN_GN_BATCH; ++k) {
            const long jk = j + k * stride;
            const long i0 = head + 4 * jk;
            const bool in = jk < n4;
            const double x = (in && (i0 < skip_lo || i0 >= skip_hi)) ? (double)v[k].x : 0.0;
            const double y = (in && (i0 + 1 < skip_lo || i0 + 1 >= skip_hi)) ? (double)v[k].y : 0.0;
            const double z = (in && (i0 + 2 < skip_lo || i0 + 2 >= skip_hi)) ? (double)v[k].z : 0.0;
            const double w = (in && (i0 + 3 < skip_lo || i0 + 3 >= skip_hi)) ? (double)v[k].w : 0.0;
            acc += x * x;
            acc += y * y;
            acc += z * z;
            acc += w * w;
        }
    }
    long e;   // scalar head and tail
    if (wn_quad_edge(qs, n, &e) && (e < skip_lo || e >= skip_hi)) acc += (double)g[e] * (double)g[e];
    acc = wn_wave_sum_f64(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int i = 1; i < (WN_TPB >> 6); ++i) s += red[i];
        partial[blockIdx.x] = s;
    }
}

int wn_grad_sumsq(const float* g, long n, long skip_lo, long skip_hi, double* partial, wn_stream_t st) {
    WN_PROF("grad_sumsq", 2.0 * (double)n, 4.0 * (double)n, st);
    if (skip_hi <= skip_lo) skip_lo = skip_hi = 0;
    WN_LAUNCH(k_grad_sumsq, dim3((unsigned)wn_grad_sumsq_blocks(n)), dim3(WN_TPB), 0, st, g, n, skip_lo, skip_hi, partial);
    return 0;
}

// One block: the partials in a fixed order, then every scalar the guarded Adam launch reads.  Everything in the state block except
// the two step counters is written from scratch (nothing depends on what the block held before).  Written once for the two
// finalize kernels; true for the one thread that wrote the block, *bc1_out = this step's 1 - beta1^steps_applied (when it applies).
static __device__ __forceinline__ bool wn_finalize_state(const double* __restrict__ partial, int nb, float max_norm, int guard,
                                                         float lr, float beta1, float beta2, WnOptState* __restrict__ state,
                                                         double* bc1_out) {
    __shared__ double red[WN_TPB >> 6];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += WN_TPB) acc += partial[i];
    acc = wn_wave_sum_f64(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return false;
    double s = red[0];
    for (int i = 1; i < (WN_TPB >> 6); ++i) s += red[i];
    // judged on the double sum (exponent field not all ones): finite elements, +-3e38 included, can never make it inf or NaN
    const bool finite = ((__builtin_bit_cast(unsigned long long, s) >> 52) & 0x7ffULL) != 0x7ffULL;
    const double norm = sqrt(s);
    // torch.nn.utils.clip_grad_norm_ (norm_type 2): min(1, max_norm / (total_norm + 1e-6)); a NaN norm gives a NaN coefficient there
    // too (the guard is what stops it).  max_norm <= 0 or inf: measure only, the coefficient is exactly 1.
    double coef = 1.0;
    if (max_norm > 0.0f && max_norm <= 3.402823466e38f) {
        coef = (double)max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    const int apply = (guard && !finite) ? 0 : 1;
    state->sumsq = s;
    state->total_norm = (float)norm;
    state->clip_coef = (float)coef;
    state->apply = apply;
    state->reserved = 0;
    state->beta1 = beta1;
    state->beta2 = beta2;
    *bc1_out = 0.0;
    if (apply) {
        const int64_t step = state->steps_applied + 1;
        state->steps_applied = step;
        // the formulas of wn_adam_step, with the device's own count of applied steps
        const double bc1 = 1.0 - pow((double)beta1, (double)step);
        const double bc2 = 1.0 - pow((double)beta2, (double)step);
        state->lr_over_bc1 = (float)((double)lr / bc1);
        state->sqrt_bc2 = (float)sqrt(bc2);
        *bc1_out = bc1;
    } else {
        state->steps_skipped = state->steps_skipped + 1;
        state->lr_over_bc1 = 0.0f;
        state->sqrt_bc2 = 0.0f;
    }
    return true;
}

__global__ __launch_bounds__(WN_TPB) void k_grad_norm_finalize(const double* __restrict__ partial, int nb, float max_norm, int guard,
                                                               float lr, float beta1, float beta2, WnOptState* __restrict__ state) {
    double bc1;
    wn_finalize_state(partial, nb, max_norm, guard, lr, beta1, beta2, state, &bc1);
}

int wn_grad_norm_finalize(const double* partial, int nb, float max_norm, int guard, float lr, float beta1, float beta2,
                          WnOptState* state, wn_stream_t st) {
    WN_PROF("grad_norm_finalize", 0.0, 8.0 * (double)nb, st);
    WN_LAUNCH(k_grad_norm_finalize, dim3(1), dim3(WN_TPB), 0, st, partial, nb, max_norm, guard, lr, beta1, beta2, state);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Adam and the sum of squares over LIVE RANGES of the flat buffers (training with frozen parameters; ABI v16).
// The table (device memory, int64, wn_live_table writes it): lo[nr], hi[nr], before[nr] -- nr sorted, disjoint, non-empty ranges
// [lo, hi) and the number of live elements in front of each.  A kernel walks the COMPACTED index space [0, n_live) with the grid
// its whole-buffer twin would use for n_live elements; compacted index c of range r is buffer element lo[r] + (c - before[r]).
// A thread finds the range of its first index by bisection, then only moves forward: while c stays inside the range it holds
// (two registers: the range's end and the offset to add) no table word is read.  Tables of up to WN_LIVE_LDS_RANGES ranges are
// staged in LDS (16 KiB) by every block; a longer one is read where it lies.  Elements outside every range are never addressed.
#define WN_LIVE_LDS_RANGES 1024
struct WnLiveTable {
    const long* lo;
    const long* before;
    int nr;
    long n_live;
};
struct WnLiveCursor {
    int r;      // the range the thread is in
    long end;   // compacted end of that range
    long off;   // buffer index = compacted index + off
};
// every thread of the block calls it (one barrier when the table is staged: nr is uniform)
static __device__ __forceinline__ WnLiveTable wn_live_stage(const long* __restrict__ table, int nr, long n_live, long* s_lo,
                                                            long* s_before) {
    if (nr > WN_LIVE_LDS_RANGES) return {table, table + 2 * (long)nr, nr, n_live};
    for (int i = threadIdx.x; i < nr; i += WN_TPB) {
        s_lo[i] = table[i];
        s_before[i] = table[2 * (long)nr + i];
    }
    __syncthreads();
    return {s_lo, s_before, nr, n_live};
}
static __device__ __forceinline__ void wn_live_enter(const WnLiveTable& t, int r, WnLiveCursor* k) {
    const long first = t.before[r];
    k->r = r;
    k->end = r + 1 < t.nr ? t.before[r + 1] : t.n_live;
    k->off = t.lo[r] - first;
}
// the last range in [r0, nr) that begins at or in front of c (c < n_live, before[r0] <= c)
static __device__ __forceinline__ void wn_live_seek(const WnLiveTable& t, long c, int r0, WnLiveCursor* k) {
    int a = r0, b = t.nr - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (t.before[mid] <= c) a = mid;
        else b = mid - 1;
    }
    wn_live_enter(t, a, k);
}
// buffer index of compacted index c, which is not in front of the cursor: the next range first (the common step), bisection over
// the ranges behind it otherwise (a stride that jumps many short ranges)
static __device__ __forceinline__ long wn_live_index(const WnLiveTable& t, long c, WnLiveCursor* k) {
    if (c >= k->end) {
        wn_live_enter(t, k->r + 1, k);
        if (c >= k->end) wn_live_seek(t, c, k->r + 1, k);
    }
    return c + k->off;
}

// One kernel for the four variants: the unguarded ones take their scalars as arguments, the guarded ones from the state block
// (and return before anything else when the step does not apply), exactly as k_adam* above.
template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(WN_TPB) void k_adam_live(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ e, const long* __restrict__ table,
                                                      int nr, long n_live, float lr_over_bc1, float sqrt_bc2, float beta1,
                                                      float beta2, float eps, float wd, float w,
                                                      const WnOptState* __restrict__ state, double ema_decay, int ema_warmup) {
    __shared__ long s_lo[WN_LIVE_LDS_RANGES], s_before[WN_LIVE_LDS_RANGES];
    float coef = 1.0f;
    if (GUARDED) {
        if (!state->apply) return;
        lr_over_bc1 = state->lr_over_bc1;
        sqrt_bc2 = state->sqrt_bc2;
        coef = state->clip_coef;
        beta1 = state->beta1;
        beta2 = state->beta2;
        if (EMA) w = wn_ema_weight(ema_decay, ema_warmup, state->steps_applied);
    }
    const WnLiveTable t = wn_live_stage(table, nr, n_live, s_lo, s_before);
    const long stride = (long)gridDim.x * WN_TPB;
    long c = (long)blockIdx.x * WN_TPB + threadIdx.x;
    if (c >= n_live) return;
    WnLiveCursor k;
    wn_live_seek(t, c, 0, &k);
    for (; c < n_live; c += stride)
        wn_adam_element<GUARDED, EMA>(p, g, m, v, e, wn_live_index(t, c, &k), lr_over_bc1, sqrt_bc2, coef, beta1, beta2, eps, wd, w);
}

template <bool GUARDED, bool EMA>
static void wn_adam_live_launch(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                                float lr_over_bc1, float sqrt_bc2, float beta1, float beta2, float eps, float wd, float w,
                                const WnOptState* state, double ema_decay, int ema_warmup, wn_stream_t st) {
    auto kernel = k_adam_live<GUARDED, EMA>;
    WN_LAUNCH(kernel, dim3(wn_adam_blocks(n_live)), dim3(WN_TPB), 0, st, p, g, m, v, e, table, nr, n_live, lr_over_bc1, sqrt_bc2,
              beta1, beta2, eps, wd, w, state, ema_decay, ema_warmup);
}

int wn_adam_live(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, float lr_over_bc1,
                 float sqrt_bc2, float beta1, float beta2, float eps, float weight_decay, float w, wn_stream_t st) {
    WN_PROF(e ? "adam_ema_live" : "adam_live", 0.0, (e ? 36.0 : 28.0) * (double)n_live, st);
    if (e) wn_adam_live_launch<false, true>(p, g, m, v, e, table, nr, n_live, lr_over_bc1, sqrt_bc2, beta1, beta2, eps, weight_decay, w, nullptr, 0.0, 0, st);
    else wn_adam_live_launch<false, false>(p, g, m, v, e, table, nr, n_live, lr_over_bc1, sqrt_bc2, beta1, beta2, eps, weight_decay, w, nullptr, 0.0, 0, st);
    return 0;
}

int wn_adam_guarded_live(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, float eps,
                         float weight_decay, const WnOptState* state, double ema_decay, int ema_warmup, wn_stream_t st) {
    WN_PROF(e ? "adam_guarded_ema_live" : "adam_guarded_live", 0.0, (e ? 36.0 : 28.0) * (double)n_live, st);
    if (e) wn_adam_live_launch<true, true>(p, g, m, v, e, table, nr, n_live, 0.0f, 0.0f, 0.0f, 0.0f, eps, weight_decay, 0.0f, state, ema_decay, ema_warmup, st);
    else wn_adam_live_launch<true, false>(p, g, m, v, e, table, nr, n_live, 0.0f, 0.0f, 0.0f, 0.0f, eps, weight_decay, 0.0f, state, ema_decay, ema_warmup, st);
    return 0;
}

// k_grad_sumsq over the live ranges: one double per block of the grid k_grad_sumsq would use for n_live elements
// (wn_grad_sumsq_blocks(n_live): a function of n_live alone), scalar loads (a range begins at any element), WN_GN_BATCH of them in
// flight per thread.  The order is fixed at every level as there -- a thread adds its elements c, c + stride, ... front to back
// -- and the products are exact in double, so the partials feed k_grad_norm_finalize unchanged and the sum is non-finite exactly
// when a live element is.
__global__ __launch_bounds__(WN_TPB) void k_grad_sumsq_live(const float* __restrict__ g, const long* __restrict__ table, int nr,
                                                            long n_live, double* __restrict__ partial) {
    __shared__ double red[WN_TPB >> 6];
    __shared__ long s_lo[WN_LIVE_LDS_RANGES], s_before[WN_LIVE_LDS_RANGES];
    const WnLiveTable t = wn_live_stage(table, nr, n_live, s_lo, s_before);
    const long stride = (long)gridDim.x * WN_TPB;
    double acc = 0.0;
    long c = (long)blockIdx.x * WN_TPB + threadIdx.x;
    if (c < n_live) {
        WnLiveCursor k;
        wn_live_seek(t, c, 0, &k);
        for (; c < n_live; c += WN_GN_BATCH * stride) {
            long idx[WN_GN_BATCH];
            float x[WN_GN_BATCH];
            WN_UNROLL
            for (int j = 0; j < WN_GN_BATCH; ++j) {
                const long cj = c + j * stride;
                idx[j] = cj < n_live ? wn_live_index(t, cj, &k) : -1;
            }
            WN_UNROLL
            for (int j = 0; j < WN_GN_BATCH; ++j) x[j] = idx[j] >= 0 ? g[idx[j]] : 0.0f;
            WN_UNROLL
            for (int j = 0; j < WN_GN_BATCH; ++j) acc += (double)x[j] * (double)x[j];
        }
    }
    acc = wn_wave_sum_f64(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = red[0];
        for (int i = 1; i < (WN_TPB >> 6); ++i) s += red[i];
        partial[blockIdx.x] = s;
    }
}

int wn_grad_sumsq_live(const float* g, const long* table, int nr, long n_live, double* partial, wn_stream_t st) {
    WN_PROF("grad_sumsq_live", 2.0 * (double)n_live, 4.0 * (double)n_live, st);
    WN_LAUNCH(k_grad_sumsq_live, dim3((unsigned)wn_grad_sumsq_blocks(n_live)), dim3(WN_TPB), 0, st, g, table, nr, n_live, partial);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Adam over PARAMETER GROUPS (ABI v17): the ranges of a live table carry a group index, table word 3 nr + r
// (wn_group_table writes it), and a group is four scalars, WnGroupScalars: lr / bc1, eps, the L2 coefficient and the decoupled
// factor.  Betas, sqrt(bc2), the clip coefficient, the apply flag and the averaging weight stay one per launch.  The grid, the
// cursor and the element are those of k_adam_live (a block's share of the compacted space is contiguous here, see below); a thread that enters a range picks up that range's four scalars and holds them
// in registers until it leaves it.  Lanes of one wave may sit in different groups, so the scalars are per-lane values: an array
// in the kernel arguments would be read by scalar loads, which a per-lane index turns into a loop over the distinct values of the
// wave.  The group block (256 bytes) is therefore staged in LDS beside the table by every block, one 16-byte read per range
// entered, and the group indices of a staged table as bytes (1 KiB, not a third more table).  The unguarded launch takes the
// block as an argument, by value: a learning rate that changes every step costs no copy.  The guarded one reads the block
// k_grad_norm_finalize_groups left in device memory.
struct WnGroupBlock {
    WnGroupScalars g[WN_MAX_PARAM_GROUPS];
};

template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(WN_TPB) void k_adam_groups(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ e, const long* __restrict__ table,
                                                        int nr, long n_live, float sqrt_bc2, float beta1, float beta2, float w,
                                                        WnGroupBlock host_block, const WnGroupScalars* __restrict__ dev_block,
                                                        const WnOptState* __restrict__ state, double ema_decay, int ema_warmup) {
    __shared__ long s_lo[WN_LIVE_LDS_RANGES], s_before[WN_LIVE_LDS_RANGES];
    __shared__ unsigned char s_group[WN_LIVE_LDS_RANGES];
    __shared__ WnGroupScalars s_block[WN_MAX_PARAM_GROUPS];
    float coef = 1.0f;
    if (GUARDED) {
        if (!state->apply) return;
        sqrt_bc2 = state->sqrt_bc2;
        coef = state->clip_coef;
        beta1 = state->beta1;
        beta2 = state->beta2;
        if (EMA) w = wn_ema_weight(ema_decay, ema_warmup, state->steps_applied);
    }
    const long* group = table + 3 * (long)nr;
    const bool staged = nr <= WN_LIVE_LDS_RANGES;
    if (threadIdx.x < WN_MAX_PARAM_GROUPS) s_block[threadIdx.x] = GUARDED ? dev_block[threadIdx.x] : host_block.g[threadIdx.x];
    if (staged)
        for (int i = threadIdx.x; i < nr; i += WN_TPB) s_group[i] = (unsigned char)group[i];
    const WnLiveTable t = wn_live_stage(table, nr, n_live, s_lo, s_before);
    if (!staged) __syncthreads();   // (wn_live_stage has no barrier of its own then)
    // A block walks ONE contiguous share of the compacted space (whole trips of the block), a thread WN_TPB elements per trip:
    // the cursor then leaves a range only where the share really crosses its end -- one step to the next range.  With the
    // grid-wide stride of k_adam_live a table of a range per tensor (biases against weights) has a thread jump several ranges
    // on nearly every trip, a bisection of dependent LDS reads each time, which at one element in flight per thread doubled
    // the launch (profiles/groups/NOTES.md).
    const long share = ((n_live + gridDim.x - 1) / gridDim.x + WN_TPB - 1) / WN_TPB * WN_TPB;
    const long last = ((long)blockIdx.x + 1) * share < n_live ? ((long)blockIdx.x + 1) * share : n_live;
    long c = (long)blockIdx.x * share + threadIdx.x;
    if (c >= last) return;
    WnLiveCursor k;
    wn_live_seek(t, c, 0, &k);
    int held = -1;
    WnGroupScalars s = {0.0f, 0.0f, 0.0f, 1.0f};
    for (; c < last; c += WN_TPB) {
        const long i = wn_live_index(t, c, &k);
        if (k.r != held) {
            held = k.r;
            s = s_block[(staged ? (int)s_group[held] : (int)group[held]) & (WN_MAX_PARAM_GROUPS - 1)];
        }
        wn_adam_element<GUARDED, EMA, true>(p, g, m, v, e, i, s.lr_over_bc1, sqrt_bc2, coef, beta1, beta2, s.eps, s.l2, w, s.scale);
    }
}

template <bool GUARDED, bool EMA>
static void wn_adam_groups_launch(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                                  float sqrt_bc2, float beta1, float beta2, float w, const WnGroupBlock& host_block,
                                  const WnGroupScalars* dev_block, const WnOptState* state, double ema_decay, int ema_warmup,
                                  wn_stream_t st) {
    auto kernel = k_adam_groups<GUARDED, EMA>;
    WN_LAUNCH(kernel, dim3(wn_adam_blocks(n_live)), dim3(WN_TPB), 0, st, p, g, m, v, e, table, nr, n_live, sqrt_bc2, beta1, beta2, w,
              host_block, dev_block, state, ema_decay, ema_warmup);
}

int wn_adam_groups(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                   const WnGroupScalars* block, float sqrt_bc2, float beta1, float beta2, float w, wn_stream_t st) {
    WN_PROF(e ? "adam_ema_groups" : "adam_groups", 0.0, (e ? 36.0 : 28.0) * (double)n_live, st);
    WnGroupBlock b;
    for (int i = 0; i < WN_MAX_PARAM_GROUPS; ++i) b.g[i] = block[i];
    if (e) wn_adam_groups_launch<false, true>(p, g, m, v, e, table, nr, n_live, sqrt_bc2, beta1, beta2, w, b, nullptr, nullptr, 0.0, 0, st);
    else wn_adam_groups_launch<false, false>(p, g, m, v, e, table, nr, n_live, sqrt_bc2, beta1, beta2, w, b, nullptr, nullptr, 0.0, 0, st);
    return 0;
}

int wn_adam_guarded_groups(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                           const WnGroupScalars* dev_block, const WnOptState* state, double ema_decay, int ema_warmup,
                           wn_stream_t st) {
    WN_PROF(e ? "adam_guarded_ema_groups" : "adam_guarded_groups", 0.0, (e ? 36.0 : 28.0) * (double)n_live, st);
    const WnGroupBlock b = {};
    if (e) wn_adam_groups_launch<true, true>(p, g, m, v, e, table, nr, n_live, 0.0f, 0.0f, 0.0f, 0.0f, b, dev_block, state, ema_decay, ema_warmup, st);
    else wn_adam_groups_launch<true, false>(p, g, m, v, e, table, nr, n_live, 0.0f, 0.0f, 0.0f, 0.0f, b, dev_block, state, ema_decay, ema_warmup, st);
    return 0;
}

// k_grad_norm_finalize with group 0's lr in the state block (the same words, bit for bit), and the group block behind it: all
// WN_MAX_PARAM_GROUPS entries are written (zeros behind n_groups); a step that does not apply leaves lr / bc1 = 0 in every group,
// as it does in the state block.
struct WnAdamGroupArgs {
    WnAdamGroup g[WN_MAX_PARAM_GROUPS];
};
__global__ __launch_bounds__(WN_TPB) void k_grad_norm_finalize_groups(const double* __restrict__ partial, int nb, float max_norm,
                                                                      int guard, WnAdamGroupArgs groups, int n_groups, float beta1,
                                                                      float beta2, WnOptState* __restrict__ state,
                                                                      WnGroupScalars* __restrict__ block) {
    double bc1;
    if (!wn_finalize_state(partial, nb, max_norm, guard, groups.g[0].lr, beta1, beta2, state, &bc1)) return;
    const bool apply = state->apply != 0;
    for (int i = 0; i < WN_MAX_PARAM_GROUPS; ++i) {
        const WnGroupScalars zero = {0.0f, 0.0f, 0.0f, 0.0f};
        block[i] = i < n_groups ? wn_group_scalars(groups.g[i], bc1, apply) : zero;
    }
}

int wn_grad_norm_finalize_groups(const double* partial, int nb, float max_norm, int guard, const WnAdamGroup* groups, int n_groups,
                                 float beta1, float beta2, WnOptState* state, WnGroupScalars* block, wn_stream_t st) {
    WN_PROF("grad_norm_finalize", 0.0, 8.0 * (double)nb, st);
    WnAdamGroupArgs a = {};
    for (int i = 0; i < n_groups; ++i) a.g[i] = groups[i];
    WN_LAUNCH(k_grad_norm_finalize_groups, dim3(1), dim3(WN_TPB), 0, st, partial, nb, max_norm, guard, a, n_groups, beta1, beta2, state,
              block);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Layer-wise adaptive steps (LAMB) and per-tensor sums of squares (ABI v20): ONE segmented reduction over the flat
// buffers.  The tensor table (wn_tensor_table writes it, int64 words): the four rows of a group table -- lo[nr], hi[nr], before[nr],
// group[nr], one range per TENSOR, never coalesced --, adapt[nr], block0[nr] = the index of the range's first block, one word for
// the number of blocks, and range_of[blocks] = the range of every block.  Every tensor owns ceil(len / WN_TENSOR_CHUNK) blocks of
// its own and block block0[r] + j walks elements [lo + j CHUNK, lo + (j + 1) CHUNK) of range r: a block lies inside ONE range,
// which it reads from range_of (one load, then the range's five words side by side: a bisection of block0 is eleven DEPENDENT
// loads at the recipe's size, and held the reduction at 1.8 TB/s), and needs neither the staged table nor the cursor of the
// kernels above.  The grid is the bound n_live / CHUNK + nr the
// launcher can form without reading the table (blocks behind the real count return at once), and every sum has a fixed order --
// per thread front to back, the xor butterfly, the waves of a block in order, the blocks of a tensor in order --: ratios are a
// function of the table, the buffers and their address modulo 16, never of the device.
struct WnTensorChunk {
    int r, group, adapt;
    long lo, len;   // the block's elements: [lo, lo + len)
};
static __device__ __forceinline__ bool wn_tensor_chunk(const long* __restrict__ table, int nr, WnTensorChunk* c) {
    const long b = blockIdx.x;
    if (b >= table[6 * (long)nr]) return false;
    const int a = (int)table[6 * (long)nr + 1 + b];
    const long lo = table[a] + (b - table[5 * (long)nr + a]) * WN_TENSOR_CHUNK, left = table[nr + a] - lo;
    c->r = a;
    c->group = (int)table[3 * (long)nr + a] & (WN_MAX_PARAM_GROUPS - 1);
    c->adapt = (int)table[4 * (long)nr + a];
    c->lo = lo;
    c->len = left < WN_TENSOR_CHUNK ? left : WN_TENSOR_CHUNK;
    return true;
}
// wn_quad_edge for a walk every block does on its own chunk: threads 0..3 own the head, 4..7 the tail
static __device__ __forceinline__ bool wn_chunk_edge(const WnQuadSplit& s, long n, long* i) {
    if (threadIdx.x >= 8) return false;
    const long t = threadIdx.x & 3;
    *i = threadIdx.x < 4 ? t : s.head + 4 * s.n4 + t;
    return *i < (threadIdx.x < 4 ? s.head : n);
}
// W = 4: one 16-byte access (the caller has checked the address), W = 1: one element
template <int W>
static __device__ __forceinline__ void wn_load(const float* a, long i, float (&x)[W]) {
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(a + i);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
        x[0] = a[i];
    }
}
template <int W>
static __device__ __forceinline__ void wn_store(float* a, long i, const float (&x)[W]) {
    if constexpr (W == 4) *reinterpret_cast<float4*>(a + i) = make_float4(x[0], x[1], x[2], x[3]);
    else a[i] = x[0];
}
// thread 0 returns the block's sum: the waves in order
static __device__ __forceinline__ double wn_block_sum_f64(double acc, double* red /*[WN_TPB >> 6]*/) {
    acc = wn_wave_sum_f64(acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < (WN_TPB >> 6); ++i) s += red[i];
    return s;
}
static __device__ __forceinline__ bool wn_same_mod16(const float* a, const float* b) {
    return ((reinterpret_cast<uintptr_t>(a) ^ reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

// what the step reads per launch: the unguarded call forms it on the host, the guarded kernels from the state block (bc1 and bc2
// by wn_bias_correction from the device's count, as the finalize launch did)
struct WnLambScalars {
    double bc1;                                  // in double: a non-adapted tensor's lr / bc1 is wn_group_scalars' quotient
    float bc1f, sqrt_bc2, coef, beta1, beta2, w;
};
template <bool GUARDED, bool EMA>
static __device__ __forceinline__ WnLambScalars wn_lamb_scalars(WnLambScalars s, const WnOptState* __restrict__ state, double ema_decay,
                                                                int ema_warmup) {
    if (GUARDED) {
        const WnBiasCorrection b = wn_bias_correction(state->beta1, state->beta2, state->steps_applied);
        s.bc1 = b.bc1;
        s.bc1f = (float)b.bc1;
        s.sqrt_bc2 = (float)sqrt(b.bc2);
        s.coef = state->clip_coef;
        s.beta1 = state->beta1;
        s.beta2 = state->beta2;
        if (EMA) s.w = wn_ema_weight(ema_decay, ema_warmup, state->steps_applied);
    }
    return s;
}
// the update direction of an adapted element from its NEW moments and its weight before the step: passes 1 and 3 both call it
static __device__ __forceinline__ float wn_lamb_update(float pv, float mv, float vv, float bc1f, float sqrt_bc2, float eps, float dwd) {
    const float u = (mv / bc1f) / (sqrtf(vv) / sqrt_bc2 + eps);
    return dwd != 0.0f ? fmaf(dwd, pv, u) : u;
}

// Pass 1.  Adapted range: the moments (wn_adam_moments: the grouped launch's bits), u, and the block's sums of p^2 and u^2 in
// double -> partial[2 b], partial[2 b + 1]; 16-byte accesses when the four buffers share their address modulo 16.  A range that
// does not adapt gets the whole grouped Adam element and is finished (its partials are neither written nor read).
// One trip of a thread: units i, i + stride, ..., at most N of them (those with an index below `end`), W elements each.  The loads
// of all N units are issued back to back before anything is computed (a unit beyond the end re-reads unit i and is dropped): a
// block is short, and with one unit in flight per thread its life was a chain of memory round trips (profiles/lamb/NOTES.md).
#define WN_TENSOR_BATCH 4
template <bool GUARDED, int W, int N>
static __device__ __forceinline__ void wn_lamb_moments_unit(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long i, long stride, long end,
                                                            const WnLambScalars& s, float eps, float l2, float dwd, double* sp,
                                                            double* su) {
    float pv[N][W], gv[N][W], mv[N][W], vv[N][W];
    WN_UNROLL
    for (int b = 0; b < N; ++b) {
        const long ib = i + b * stride < end ? i + b * stride : i;
        wn_load<W>(p, ib, pv[b]);
        wn_load<W>(g, ib, gv[b]);
        wn_load<W>(m, ib, mv[b]);
        wn_load<W>(v, ib, vv[b]);
    }
    WN_UNROLL
    for (int b = 0; b < N; ++b) {
        if (i + b * stride >= end) break;
        WN_UNROLL
        for (int k = 0; k < W; ++k) {
            wn_adam_moments<GUARDED>(pv[b][k], gv[b][k], mv[b][k], vv[b][k], s.coef, s.beta1, s.beta2, l2, &mv[b][k], &vv[b][k]);
            const float u = wn_lamb_update(pv[b][k], mv[b][k], vv[b][k], s.bc1f, s.sqrt_bc2, eps, dwd);
            *sp += (double)pv[b][k] * (double)pv[b][k];
            *su += (double)u * (double)u;
        }
        wn_store<W>(m, i + b * stride, mv[b]);
        wn_store<W>(v, i + b * stride, vv[b]);
    }
}

template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(WN_TPB) void k_lamb_moments(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, float* __restrict__ e, const long* __restrict__ table,
                                                         int nr, WnLambScalars s, WnAdamGroupArgs groups, WnGroupBlock host_block,
                                                         const WnOptState* __restrict__ state, double ema_decay, int ema_warmup,
                                                         double* __restrict__ partial) {
    __shared__ double red_p[WN_TPB >> 6], red_u[WN_TPB >> 6];
    if (GUARDED && !state->apply) return;
    WnTensorChunk c;
    if (!wn_tensor_chunk(table, nr, &c)) return;
    s = wn_lamb_scalars<GUARDED, EMA>(s, state, ema_decay, ema_warmup);
    const WnAdamGroup a = groups.g[c.group];
    if (!c.adapt) {
        const WnGroupScalars gs = GUARDED ? wn_group_scalars(a, s.bc1, true) : host_block.g[c.group];
        for (long i = c.lo + threadIdx.x; i < c.lo + c.len; i += WN_TPB)
            wn_adam_element<GUARDED, EMA, true>(p, g, m, v, e, i, gs.lr_over_bc1, s.sqrt_bc2, s.coef, s.beta1, s.beta2, gs.eps, gs.l2, s.w,
                                                gs.scale);
        return;
    }
    const float l2 = a.decoupled ? 0.0f : a.weight_decay, dwd = a.decoupled ? a.weight_decay : 0.0f;
    double sp = 0.0, su = 0.0;
    if (wn_same_mod16(p, g) && wn_same_mod16(p, m) && wn_same_mod16(p, v)) {
        const WnQuadSplit qs = wn_quad_split(p + c.lo, c.len);
        const long q0 = c.lo + qs.head, q1 = q0 + 4 * qs.n4;
        for (long i = q0 + 4 * threadIdx.x; i < q1; i += WN_TENSOR_BATCH * 4 * WN_TPB)
            wn_lamb_moments_unit<GUARDED, 4, WN_TENSOR_BATCH>(p, g, m, v, i, 4 * WN_TPB, q1, s, a.eps, l2, dwd, &sp, &su);
        long i;
        if (wn_chunk_edge(qs, c.len, &i)) wn_lamb_moments_unit<GUARDED, 1, 1>(p, g, m, v, c.lo + i, 0, c.lo + c.len, s, a.eps, l2, dwd, &sp, &su);
    } else {
        const long end = c.lo + c.len;
        for (long i = c.lo + threadIdx.x; i < end; i += WN_TENSOR_BATCH * WN_TPB)
            wn_lamb_moments_unit<GUARDED, 1, WN_TENSOR_BATCH>(p, g, m, v, i, WN_TPB, end, s, a.eps, l2, dwd, &sp, &su);
    }
    sp = wn_block_sum_f64(sp, red_p);
    su = wn_block_sum_f64(su, red_u);
    if (threadIdx.x == 0) {
        partial[2 * (long)blockIdx.x] = sp;
        partial[2 * (long)blockIdx.x + 1] = su;
    }
}

// Pass 2: one thread per tensor adds its blocks' partials in block order and writes ||w||, ||u|| and the trust ratio (three
// floats per tensor).  ||w|| == 0 or ||u|| == 0: ratio 1; a non-finite norm (guard off) stays in the ratio.  max_trust > 0 clamps.
__global__ __launch_bounds__(WN_TPB) void k_lamb_ratios(const double* __restrict__ partial, const long* __restrict__ table, int nr,
                                                        float max_trust, const WnOptState* __restrict__ state,
                                                        float* __restrict__ stats) {
    if (state && !state->apply) return;
    const int r = blockIdx.x * WN_TPB + threadIdx.x;
    if (r >= nr) return;
    float wn = 0.0f, un = 0.0f, ratio = 1.0f;
    if (table[4 * (long)nr + r]) {
        const long b0 = table[5 * (long)nr + r], b1 = r + 1 < nr ? table[5 * (long)nr + r + 1] : table[6 * (long)nr];
        double sp = 0.0, su = 0.0;
        for (long b = b0; b < b1; ++b) {
            sp += partial[2 * b];
            su += partial[2 * b + 1];
        }
        const double w2 = sqrt(sp), u2 = sqrt(su);
        wn = (float)w2;
        un = (float)u2;
        if (!(w2 == 0.0) && !(u2 == 0.0)) ratio = (float)(w2 / u2);
        if (max_trust > 0.0f && ratio > max_trust) ratio = max_trust;
    }
    stats[3 * (long)r] = wn;
    stats[3 * (long)r + 1] = un;
    stats[3 * (long)r + 2] = ratio;
}

// Pass 3, adapted ranges only: u again from the stored moments and the weight (wn_lamb_update, as pass 1), p -= (lr_g r) u and
// the moving average.  No n-sized temporary: 10 words per element over the two passes.
template <bool EMA, int W, int N>
static __device__ __forceinline__ void wn_lamb_apply_unit(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                          float* __restrict__ e, long i, long stride, long end, const WnLambScalars& s,
                                                          float eps, float dwd, float step) {
    float pv[N][W], mv[N][W], vv[N][W], ev[N][W];
    WN_UNROLL
    for (int b = 0; b < N; ++b) {
        const long ib = i + b * stride < end ? i + b * stride : i;
        wn_load<W>(p, ib, pv[b]);
        wn_load<W>(m, ib, mv[b]);
        wn_load<W>(v, ib, vv[b]);
        if (EMA) wn_load<W>(e, ib, ev[b]);
    }
    WN_UNROLL
    for (int b = 0; b < N; ++b) {
        if (i + b * stride >= end) break;
        WN_UNROLL
        for (int k = 0; k < W; ++k) {
            const float u = wn_lamb_update(pv[b][k], mv[b][k], vv[b][k], s.bc1f, s.sqrt_bc2, eps, dwd);
            pv[b][k] = fmaf(-step, u, pv[b][k]);
            if (EMA) ev[b][k] = fmaf(s.w, pv[b][k] - ev[b][k], ev[b][k]);
        }
        wn_store<W>(p, i + b * stride, pv[b]);
        if (EMA) wn_store<W>(e, i + b * stride, ev[b]);
    }
}

template <bool GUARDED, bool EMA>
__global__ __launch_bounds__(WN_TPB) void k_lamb_apply(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                       float* __restrict__ e, const long* __restrict__ table, int nr, WnLambScalars s,
                                                       WnAdamGroupArgs groups, const WnOptState* __restrict__ state, double ema_decay,
                                                       int ema_warmup, const float* __restrict__ stats) {
    if (GUARDED && !state->apply) return;
    WnTensorChunk c;
    if (!wn_tensor_chunk(table, nr, &c) || !c.adapt) return;
    s = wn_lamb_scalars<GUARDED, EMA>(s, state, ema_decay, ema_warmup);
    const WnAdamGroup a = groups.g[c.group];
    const float dwd = a.decoupled ? a.weight_decay : 0.0f;
    const float step = wn_fmul_rn(a.lr, stats[3 * (long)c.r + 2]);
    if (wn_same_mod16(p, m) && wn_same_mod16(p, v) && (!EMA || wn_same_mod16(p, e))) {
        const WnQuadSplit qs = wn_quad_split(p + c.lo, c.len);
        const long q0 = c.lo + qs.head, q1 = q0 + 4 * qs.n4;
        for (long i = q0 + 4 * threadIdx.x; i < q1; i += WN_TENSOR_BATCH * 4 * WN_TPB)
            wn_lamb_apply_unit<EMA, 4, WN_TENSOR_BATCH>(p, m, v, e, i, 4 * WN_TPB, q1, s, a.eps, dwd, step);
        long i;
        if (wn_chunk_edge(qs, c.len, &i)) wn_lamb_apply_unit<EMA, 1, 1>(p, m, v, e, c.lo + i, 0, c.lo + c.len, s, a.eps, dwd, step);
    } else {
        const long end = c.lo + c.len;
        for (long i = c.lo + threadIdx.x; i < end; i += WN_TENSOR_BATCH * WN_TPB)
            wn_lamb_apply_unit<EMA, 1, WN_TENSOR_BATCH>(p, m, v, e, i, WN_TPB, end, s, a.eps, dwd, step);
    }
}

static unsigned wn_tensor_grid(int nr, long n_live) { return (unsigned)(n_live / WN_TENSOR_CHUNK + nr); }

template <bool GUARDED, bool EMA>
static void wn_lamb_launch(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live,
                           const WnLambScalars& s, const WnAdamGroupArgs& groups, const WnGroupBlock& block, float max_trust,
                           const WnOptState* state, double ema_decay, int ema_warmup, double* partial, float* stats, wn_stream_t st) {
    const dim3 grid(wn_tensor_grid(nr, n_live));
    auto moments = k_lamb_moments<GUARDED, EMA>;
    auto apply = k_lamb_apply<GUARDED, EMA>;
    {
        WN_PROF("lamb_moments", 0.0, 24.0 * (double)n_live, st);
        WN_LAUNCH(moments, grid, dim3(WN_TPB), 0, st, p, g, m, v, e, table, nr, s, groups, block, state, ema_decay, ema_warmup, partial);
    }
    {
        WN_PROF("lamb_ratios", 0.0, 16.0 * (double)grid.x, st);
        WN_LAUNCH(k_lamb_ratios, dim3((unsigned)((nr + WN_TPB - 1) / WN_TPB)), dim3(WN_TPB), 0, st, partial, table, nr, max_trust, state,
                  stats);
    }
    {
        WN_PROF("lamb_apply", 0.0, (EMA ? 24.0 : 16.0) * (double)n_live, st);
        WN_LAUNCH(apply, grid, dim3(WN_TPB), 0, st, p, m, v, e, table, nr, s, groups, state, ema_decay, ema_warmup, stats);
    }
}

int wn_lamb(float* p, const float* g, float* m, float* v, float* e, const long* table, int nr, long n_live, long step,
            const WnAdamGroup* groups, int n_groups, float beta1, float beta2, float max_trust, const WnOptState* state,
            double ema_decay, int ema_warmup, double* partial, float* stats, wn_stream_t st) {
    WnAdamGroupArgs a = {};
    WnGroupBlock block = {};
    WnLambScalars s = {};
    s.coef = 1.0f;
    if (!state) {
        const WnBiasCorrection b = wn_bias_correction(beta1, beta2, step);
        s.bc1 = b.bc1;
        s.bc1f = (float)b.bc1;
        s.sqrt_bc2 = (float)sqrt(b.bc2);
        s.beta1 = beta1;
        s.beta2 = beta2;
        if (e) s.w = wn_ema_weight(ema_decay, ema_warmup, step);
    }
    for (int i = 0; i < n_groups; ++i) {
        a.g[i] = groups[i];
        if (!state) block.g[i] = wn_group_scalars(groups[i], s.bc1, true);
    }
    if (state) {
        if (e) wn_lamb_launch<true, true>(p, g, m, v, e, table, nr, n_live, s, a, block, max_trust, state, ema_decay, ema_warmup, partial, stats, st);
        else wn_lamb_launch<true, false>(p, g, m, v, e, table, nr, n_live, s, a, block, max_trust, state, ema_decay, ema_warmup, partial, stats, st);
    } else {
        if (e) wn_lamb_launch<false, true>(p, g, m, v, e, table, nr, n_live, s, a, block, max_trust, state, ema_decay, ema_warmup, partial, stats, st);
        else wn_lamb_launch<false, false>(p, g, m, v, e, table, nr, n_live, s, a, block, max_trust, state, ema_decay, ema_warmup, partial, stats, st);
    }
    return 0;
}

// The same segmented reduction for any flat fp32 buffer: out[r] = the sum of x[i]^2 over range r, in double.
__global__ __launch_bounds__(WN_TPB) void k_tensor_sumsq(const float* __restrict__ x, const long* __restrict__ table, int nr,
                                                         double* __restrict__ partial) {
    __shared__ double red[WN_TPB >> 6];
    WnTensorChunk c;
    if (!wn_tensor_chunk(table, nr, &c)) return;
    double acc = 0.0;
    const WnQuadSplit qs = wn_quad_split(x + c.lo, c.len);
    const long q0 = c.lo + qs.head, q1 = q0 + 4 * qs.n4;
    for (long j = q0 + 4 * threadIdx.x; j < q1; j += WN_TENSOR_BATCH * 4 * WN_TPB) {
        float q[WN_TENSOR_BATCH][4];
        WN_UNROLL
        for (int b = 0; b < WN_TENSOR_BATCH; ++b) wn_load<4>(x, j + b * 4 * WN_TPB < q1 ? j + b * 4 * WN_TPB : j, q[b]);
        WN_UNROLL
        for (int b = 0; b < WN_TENSOR_BATCH; ++b) {
            if (j + b * 4 * WN_TPB >= q1) break;
            WN_UNROLL
            for (int k = 0; k < 4; ++k) acc += (double)q[b][k] * (double)q[b][k];
        }
    }
    long i;
    if (wn_chunk_edge(qs, c.len, &i)) acc += (double)x[c.lo + i] * (double)x[c.lo + i];
    acc = wn_block_sum_f64(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(WN_TPB) void k_tensor_sums(const double* __restrict__ partial, const long* __restrict__ table, int nr,
                                                        double* __restrict__ out) {
    const int r = blockIdx.x * WN_TPB + threadIdx.x;
    if (r >= nr) return;
    const long b0 = table[5 * (long)nr + r], b1 = r + 1 < nr ? table[5 * (long)nr + r + 1] : table[6 * (long)nr];
    double s = 0.0;
    for (long b = b0; b < b1; ++b) s += partial[b];
    out[r] = s;
}

int wn_tensor_sumsq_launch(const float* x, const long* table, int nr, long n_live, double* partial, double* out, wn_stream_t st) {
    {
        WN_PROF("tensor_sumsq", 2.0 * (double)n_live, 4.0 * (double)n_live, st);
        WN_LAUNCH(k_tensor_sumsq, dim3(wn_tensor_grid(nr, n_live)), dim3(WN_TPB), 0, st, x, table, nr, partial);
    }
    WN_PROF("tensor_sums", 0.0, 8.0 * (double)nr, st);
    WN_LAUNCH(k_tensor_sums, dim3((unsigned)((nr + WN_TPB - 1) / WN_TPB)), dim3(WN_TPB), 0, st, partial, table, nr, out);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// One walk over two non-overlapping buffers a and b (the entry points refuse an overlap, so every element is read and written
// by exactly one thread), one OP per element.  When a and b share their address modulo 16 the body moves 16-byte quads (BATCH
// of each buffer in flight per thread) behind a scalar head and in front of a scalar tail; otherwise every element goes alone.
// OP names what it needs: b is always read, a only with READ_A, and WRITE_A / WRITE_B say which side apply() changed.
//   WnSwapOp                   a[i] <-> b[i] with no temporary buffer
//   WnAccumOp<WN_ACCUM_SET>    a[i] = b[i]            gradient accumulation over micro-batches (include/wavenet_hip.h, ABI v15),
//   WnAccumOp<WN_ACCUM_ADD>    a[i] = a[i] + b[i]     a = acc, b = grad: one plain fp32 add per element, nothing else
//   WnAccumOp<WN_ACCUM_FINISH> b[i] = a[i] + b[i]
struct WnSwapOp {
    static constexpr bool READ_A = true, WRITE_A = true, WRITE_B = true;
    static __device__ __forceinline__ void apply(float& a, float& b) {
        const float t = a;
        a = b;
        b = t;
    }
};
template <int MODE>
struct WnAccumOp {
    static constexpr bool READ_A = MODE != WN_ACCUM_SET, WRITE_A = MODE != WN_ACCUM_FINISH, WRITE_B = MODE == WN_ACCUM_FINISH;
    static __device__ __forceinline__ void apply(float& a, float& b) {
        const float s = READ_A ? a + b : b;
        if (WRITE_B) b = s;
        else a = s;
    }
};

template <class OP>
static __device__ __forceinline__ void wn_pair_one(float* a, float* b, long i) {
    float y = b[i], x = OP::READ_A ? a[i] : 0.0f;
    OP::apply(x, y);
    if (OP::WRITE_A) a[i] = x;
    if (OP::WRITE_B) b[i] = y;
}

template <class OP, int BATCH>
static __device__ __forceinline__ void wn_pair_sweep(float* a, float* b, long n) {
    const long stride = (long)gridDim.x * WN_TPB;
    const long tid = (long)blockIdx.x * WN_TPB + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(a) & 15) != (reinterpret_cast<uintptr_t>(b) & 15)) {
        for (long i = tid; i < n; i += stride) wn_pair_one<OP>(a, b, i);
        return;
    }
    const WnQuadSplit s = wn_quad_split(a, n);
    float4* a4 = reinterpret_cast<float4*>(a + s.head);
    float4* b4 = reinterpret_cast<float4*>(b + s.head);
    for (long j = tid; j < s.n4; j += BATCH * stride) {
        float4 x[BATCH], y[BATCH];   // x stays unset without READ_A: such an OP's apply() may assign its `a`, never read it
        WN_UNROLL
        for (int k = 0; k < BATCH; ++k) {
            const long jk = j + k * stride;
            if (jk < s.n4) {
                y[k] = b4[jk];
                if (OP::READ_A) x[k] = a4[jk];
            }
        }
        WN_UNROLL
        for (int k = 0; k < BATCH; ++k) {
            const long jk = j + k * stride;
            if (jk < s.n4) {
                OP::apply(x[k].x, y[k].x);
                OP::apply(x[k].y, y[k].y);
                OP::apply(x[k].z, y[k].z);
                OP::apply(x[k].w, y[k].w);
                if (OP::WRITE_A) a4[jk] = x[k];
                if (OP::WRITE_B) b4[jk] = y[k];
            }
        }
    }
    long i;
    if (wn_quad_edge(s, n, &i)) wn_pair_one<OP>(a, b, i);
}

#define WN_SWAP_MAXBLOCKS 512
#define WN_SWAP_BATCH 2
__global__ __launch_bounds__(WN_TPB) void k_swap(float* a, float* b, long n) { wn_pair_sweep<WnSwapOp, WN_SWAP_BATCH>(a, b, n); }

int wn_swap(float* a, float* b, long n, wn_stream_t st) {
    WN_PROF("swap", 0.0, 16.0 * (double)n, st);
    WN_LAUNCH(k_swap, dim3(wn_quad_blocks(n, WN_SWAP_MAXBLOCKS)), dim3(WN_TPB), 0, st, a, b, n);
    return 0;
}

#define WN_ACCUM_MAXBLOCKS 1024
#define WN_ACCUM_BATCH 2
template <int MODE>
__global__ __launch_bounds__(WN_TPB) void k_grad_accumulate(float* __restrict__ acc, float* __restrict__ grad, long n) {
    wn_pair_sweep<WnAccumOp<MODE>, WN_ACCUM_BATCH>(acc, grad, n);
}

int wn_grad_accumulate(float* acc, float* grad, long n, int mode, wn_stream_t st) {
    if (mode != WN_ACCUM_SET && mode != WN_ACCUM_ADD && mode != WN_ACCUM_FINISH) return 1;
    WN_PROF("grad_accumulate", 0.0, 12.0 * (double)n, st);
    const dim3 grid(wn_quad_blocks(n, WN_ACCUM_MAXBLOCKS));
    if (mode == WN_ACCUM_SET) {
        WN_LAUNCH(k_grad_accumulate<WN_ACCUM_SET>, grid, dim3(WN_TPB), 0, st, acc, grad, n);
    } else if (mode == WN_ACCUM_ADD) {
        WN_LAUNCH(k_grad_accumulate<WN_ACCUM_ADD>, grid, dim3(WN_TPB), 0, st, acc, grad, n);
    } else {
        WN_LAUNCH(k_grad_accumulate<WN_ACCUM_FINISH>, grid, dim3(WN_TPB), 0, st, acc, grad, n);
    }
    return 0;
}
