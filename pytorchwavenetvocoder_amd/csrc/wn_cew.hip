// wn_cew.hip -- the weighted cross-entropy head of the softmax model: one weight per class, label smoothing and one weight per
// position (torch's CrossEntropyLoss(weight=, label_smoothing=) plus a (B, T) weight), with its gradient with respect to the
// logits (gfx950).  The definition is in wn_cew.h.
//
// The shape of k_softmax_distill (wn_distill.hip) with one input: for Q <= 256 a workgroup of 4 waves covers 64 consecutive
// positions, wave w keeps the classes [w * ceil(Q / 4), ..) of those positions in registers -- at most 64 values per lane -- and
// the logits are read once, 64 consecutive t per instruction (256 B).  The column maximum, sum exp, sum_q w_q (s_q - max) and
// s_y - max cross the 4 waves through LDS, dlogits is written from the registers.  The class weights are wave-uniform per
// register index: each wave parks its own quarter of them in LDS and reads them back as broadcasts.
//
// Arithmetic (k_softmax_ce, k_softmax_distill): log-probabilities are differences against the column maximum,
// log p_q = (s_q - max) - log(sum exp), never formed through log(sum) + max; sums run in 4 interleaved accumulators added as a
// tree.  sum_q w_q (-log p_q) = W log(sum exp) - sum_q w_q (s_q - max): both terms are sums of non-negative numbers.  Nothing
// is clamped: a -inf class with eps > 0 and w_q > 0 gives l = +inf, a class with w_q == 0 is left out of the sum (0 * inf).
#include "wn_cew.h"
#include "wn_prof.h"

#include <math.h>
#include <stdlib.h>

#define WC_POS 64     // positions per workgroup (one per lane)
#define WC_TPB 256    // 4 waves: a quarter of the classes each
#define WC_DPOS 1024  // positions per workgroup of k_ce_divisor (4 per thread)

// max(a, |v|) on the bit patterns: inf and NaN stay on top (the fp16 pair split of the backward pass then takes its redo)
static __device__ __forceinline__ float wc_absmax(float a, float v) {
    const int ai = __builtin_bit_cast(int, a), vi = __builtin_bit_cast(int, v) & 0x7fffffff;
    return __builtin_bit_cast(float, vi > ai ? vi : ai);
}
static __device__ __forceinline__ float wc_wave_absmax(float a) {
    int ai = __builtin_bit_cast(int, a);
    WN_UNROLL
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(ai, m, 64); ai = o > ai ? o : ai; }
    return __builtin_bit_cast(float, ai);
}
static __device__ __forceinline__ float wc_tree4(const float* v) { return (v[0] + v[1]) + (v[2] + v[3]); }

struct WcArgs {
    const float* s;         // logits (B, Q, T)
    const int64_t* target;  // (B, T)
    const float* cw;        // (Q) class weights or NULL (ones)
    const float* r;         // (B, T) position weights or NULL (ones)
    float* dlogits;         // (B, Q, T) or NULL
    float* pos_loss;        // (B, T) or NULL
    float* part;            // [3][B][nblk]: sums of r l, sums of ce, max |dlogits|
    const int* t_end;       // (B) or NULL
    const double* dw;       // {D, 1 / D} left by k_ce_divisor_tail, or NULL: inv_d below
    double inv_d;           // 1 / D known on the host ("positions", or no weight of either kind)
    int T, Q, t_start, qw;  // qw = ceil(Q / 4): classes per wave
    float eps, gs;
};

static __device__ __forceinline__ int wc_class(const int64_t* target, long at, int Q) {   // class index modulo Q like k_softmax_ce
    long long tg = target[at] % Q;
    if (tg < 0) tg += Q;
    return (int)tg;
}

// l of one position from its column sums: lz = log(sum exp(s - max)), ce = lz - (s_y - max), sw = sum_q w_q (s_q - max)
static __device__ __forceinline__ float wc_position(const WcArgs& a, float wy, float ce, float lz, float W, float sw) {
    const float hard = ((1.0f - a.eps) * wy) * ce;
    return a.eps == 0.0f ? hard : hard + (a.eps / (float)a.Q) * (W * lz - sw);
}

template <int NQ>
__global__ __launch_bounds__(WC_TPB) void k_softmax_cew(const WcArgs a) {
    __shared__ float cw_s[4][WC_POS];
    __shared__ float red_max[4][WC_POS];
    __shared__ float red_sum[2][4][WC_POS];
    __shared__ float red_sy[WC_POS];
    __shared__ float red_w[4];
    __shared__ float red_amax[4];
    const int lane = threadIdx.x & 63, w = WN_UNIFORM(threadIdx.x >> 6);
    const int b = blockIdx.y, T = a.T, Q = a.Q;
    const int t0 = blockIdx.x * WC_POS, t = t0 + lane;
    const int te = (a.t_end && a.t_end[b] < T) ? a.t_end[b] : T;   // ragged batch: the sequence's own end (block-uniform)
    const bool live = t >= a.t_start && t < te;
    const int q0 = w * a.qw;
    const int qn = Q - q0 < a.qw ? (Q - q0 < 0 ? 0 : Q - q0) : a.qw;   // classes of this wave (wave-uniform)
    // buffer access (wn_device.h): the wave's rows are one buffer of qn * T floats, a row is a wave-uniform offset and the
    // position the only per-lane address register; lanes that must not read or write carry an offset past the buffer
    const long row0 = ((long)b * Q + q0) * T;
    const unsigned rows_bytes = (unsigned)qn * (unsigned)T * 4u;
    const wn_rsrc_t bs_ = wn_make_buf(a.s + row0, rows_bytes);
    const wn_rsrc_t bd_ = wn_make_buf(a.dlogits != nullptr ? a.dlogits + row0 : a.s, a.dlogits != nullptr ? rows_bytes : 0u);
    const int v_ld = live ? t * 4 : WN_VOFF_DEAD, v_st = t < T ? t * 4 : WN_VOFF_DEAD;
    const int row_bytes = T * 4;
    const int pidx = blockIdx.y * gridDim.x + blockIdx.x, pn = gridDim.x * gridDim.y;
    if (t0 + WC_POS <= a.t_start || t0 >= te) {   // no live position in the block: zeros out, no logit read
        if (a.dlogits != nullptr)
            for (int i = 0; i < qn; ++i) wn_buf_store(bd_, 0.0f, v_st, i * row_bytes);
        if (w == 0 && a.pos_loss != nullptr && t < T) a.pos_loss[(long)b * T + t] = 0.0f;
        if (threadIdx.x == 0) {
            a.part[pidx] = 0.0f;
            a.part[pn + pidx] = 0.0f;
            if (a.dlogits != nullptr) a.part[2 * pn + pidx] = 0.0f;
        }
        return;
    }
    const bool smooth = a.eps != 0.0f;   // (uniform)
    // the wave's own quarter of the class weights, read back below as broadcasts (slots past the wave's classes are not read)
    if (smooth) cw_s[w][lane] = lane < qn ? (a.cw != nullptr ? a.cw[q0 + lane] : 1.0f) : 0.0f;
    // the wave's quarter of the column, read once; slots past the wave's classes hold -inf (exp -> 0), dead positions read
    // nothing (their lanes compute on zeros and contribute nowhere)
    float s[NQ];
    WN_UNROLL
    for (int i = 0; i < NQ; ++i) s[i] = i < qn ? wn_buf_load_once(bs_, v_ld, i * row_bytes) : -INFINITY;
    float ms = -INFINITY;
    WN_UNROLL
    for (int i = 0; i < NQ; ++i) ms = fmaxf(ms, s[i]);
    red_max[w][lane] = ms;
    __syncthreads();
    ms = fmaxf(fmaxf(red_max[0][lane], red_max[1][lane]), fmaxf(red_max[2][lane], red_max[3][lane]));
    const int y = live ? wc_class(a.target, (long)b * T + t, Q) : -1;
    const int yl = y - q0;   // the target's register index in this wave, outside [0, qn) in the three others
    // four interleaved accumulators per sum, added as a tree: a chain of 16 terms at most, not of 64
    float Za[4] = {0.0f, 0.0f, 0.0f, 0.0f}, swa[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Wa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float sy = 0.0f;
    if (smooth) {
        WN_UNROLL
        for (int i = 0; i < NQ; ++i) {
            if (i < qn) {
                const float as = s[i] - ms, wq = cw_s[w][i];
                Wa[i & 3] += wq;
                if (wq != 0.0f) swa[i & 3] += wq * as;
                if (i == yl) sy = as;
                s[i] = expf(as);   // softmax numerators from here on
                Za[i & 3] += s[i];
            }
        }
    } else {
        WN_UNROLL
        for (int i = 0; i < NQ; ++i) {
            if (i < qn) {
                const float as = s[i] - ms;
                if (i == yl) sy = as;
                s[i] = expf(as);
                Za[i & 3] += s[i];
            }
        }
    }
    float Z = wc_tree4(Za), sw = wc_tree4(swa), W = wc_tree4(Wa);
    red_sum[0][w][lane] = Z;
    red_sum[1][w][lane] = sw;
    if (yl >= 0 && yl < qn) red_sy[lane] = sy;   // (one wave per live position)
    if (lane == 0) red_w[w] = W;
    __syncthreads();
    Z = (red_sum[0][0][lane] + red_sum[0][1][lane]) + (red_sum[0][2][lane] + red_sum[0][3][lane]);
    sw = (red_sum[1][0][lane] + red_sum[1][1][lane]) + (red_sum[1][2][lane] + red_sum[1][3][lane]);
    W = (red_w[0] + red_w[1]) + (red_w[2] + red_w[3]);
    // position weight, the target's class weight and the position's factor on the gradient, grad_scale r / D: the two per-lane
    // gathers of the kernel.  A position with r == 0, and every position with D == 0, is off: exact zeros.
    const float rr = live ? (a.r != nullptr ? a.r[(long)b * T + t] : 1.0f) : 0.0f;
    const float wy = live ? (a.cw != nullptr ? a.cw[y] : 1.0f) : 0.0f;
    const float coef = (float)(((double)a.gs * (double)rr) * (a.dw != nullptr ? a.dw[1] : a.inv_d));
    if (w == 0) {
        float ce = 0.0f, rl = 0.0f;
        if (live) {
            const float lz = logf(Z);
            ce = lz - red_sy[lane];
            if (rr != 0.0f) rl = rr * wc_position(a, wy, ce, lz, W, sw);
        }
        if (a.pos_loss != nullptr && t < T) a.pos_loss[(long)b * T + t] = rl;
        const float trl = wave_reduce_sum(rl), tce = wave_reduce_sum(ce);
        if (lane == 0) {
            a.part[pidx] = trl;
            a.part[pn + pidx] = tce;
        }
    }
    if (a.dlogits == nullptr) return;
    float amax = 0.0f;
    if (live && coef != 0.0f) {
        const float rz = 1.0f / Z;
        // grad_scale r / D goes into the three factors that carry the weights, not onto the finished g: a common power of two
        // on w then cancels in hk, sW and sk w_q themselves, and dlogits keeps its bits even where p_q is subnormal
        const float hk = ((1.0f - a.eps) * wy) * coef, sk = (a.eps / (float)Q) * coef, sW = sk * W;
        if (smooth) {
            WN_UNROLL
            for (int i = 0; i < NQ; ++i) {
                if (i < qn) {
                    const float p = s[i] * rz;
                    const float d = hk * (p - (i == yl ? 1.0f : 0.0f)) + (sW * p - sk * cw_s[w][i]);
                    wn_buf_store(bd_, d, v_st, i * row_bytes);
                    amax = wc_absmax(amax, d);
                }
            }
        } else {
            WN_UNROLL
            for (int i = 0; i < NQ; ++i) {
                if (i < qn) {
                    const float d = hk * (s[i] * rz - (i == yl ? 1.0f : 0.0f));
                    wn_buf_store(bd_, d, v_st, i * row_bytes);
                    amax = wc_absmax(amax, d);
                }
            }
        }
    } else {
        for (int i = 0; i < qn; ++i) wn_buf_store(bd_, 0.0f, v_st, i * row_bytes);
    }
    amax = wc_wave_absmax(amax);
    if (lane == 0) red_amax[w] = amax;
    __syncthreads();
    if (threadIdx.x == 0) a.part[2 * pn + pidx] = wc_absmax(wc_absmax(red_amax[0], red_amax[1]), wc_absmax(red_amax[2], red_amax[3]));
}

// More than 256 classes: one thread per position, plain loops over the column (three reads of it).  Same partials.
__global__ __launch_bounds__(WC_POS) void k_softmax_cew_wide(const WcArgs a) {
    const int lane = threadIdx.x;
    const int b = blockIdx.y, T = a.T, Q = a.Q;
    const int t = blockIdx.x * WC_POS + lane;
    const int te = (a.t_end && a.t_end[b] < T) ? a.t_end[b] : T;
    const bool live = t >= a.t_start && t < te;
    const long col = (long)b * Q * T + t;
    const int pidx = blockIdx.y * gridDim.x + blockIdx.x, pn = gridDim.x * gridDim.y;
    float ce = 0.0f, rl = 0.0f, amax = 0.0f;
    bool written = false;
    if (live) {
        const float* sp = a.s + col;
        const bool smooth = a.eps != 0.0f;
        float ms = -INFINITY;
        for (int q = 0; q < Q; ++q) ms = fmaxf(ms, sp[(long)q * T]);
        // eight interleaved accumulators per sum, added as a tree
        float Za[8], swa[8], Wa[8];
        for (int k = 0; k < 8; ++k) Za[k] = swa[k] = Wa[k] = 0.0f;
        for (int q = 0; q < Q; ++q) {
            const float as = sp[(long)q * T] - ms;
            Za[q & 7] += expf(as);
            if (smooth) {
                const float wq = a.cw != nullptr ? a.cw[q] : 1.0f;
                Wa[q & 7] += wq;
                if (wq != 0.0f) swa[q & 7] += wq * as;
            }
        }
        const float Z = ((Za[0] + Za[1]) + (Za[2] + Za[3])) + ((Za[4] + Za[5]) + (Za[6] + Za[7]));
        const float sw = ((swa[0] + swa[1]) + (swa[2] + swa[3])) + ((swa[4] + swa[5]) + (swa[6] + swa[7]));
        const float W = ((Wa[0] + Wa[1]) + (Wa[2] + Wa[3])) + ((Wa[4] + Wa[5]) + (Wa[6] + Wa[7]));
        const int y = wc_class(a.target, (long)b * T + t, Q);
        const float rr = a.r != nullptr ? a.r[(long)b * T + t] : 1.0f;
        const float wy = a.cw != nullptr ? a.cw[y] : 1.0f;
        const float coef = (float)(((double)a.gs * (double)rr) * (a.dw != nullptr ? a.dw[1] : a.inv_d));
        const float lz = logf(Z);
        ce = lz - (sp[(long)y * T] - ms);
        if (rr != 0.0f) rl = rr * wc_position(a, wy, ce, lz, W, sw);
        if (a.dlogits != nullptr && coef != 0.0f) {
            const float rz = 1.0f / Z;
            const float hk = ((1.0f - a.eps) * wy) * coef, sk = (a.eps / (float)Q) * coef, sW = sk * W;   // (as k_softmax_cew)
            for (int q = 0; q < Q; ++q) {
                const float p = expf(sp[(long)q * T] - ms) * rz;
                float d = hk * (p - (q == y ? 1.0f : 0.0f));
                if (smooth) d += sW * p - sk * (a.cw != nullptr ? a.cw[q] : 1.0f);
                a.dlogits[col + (long)q * T] = d;
                amax = wc_absmax(amax, d);
            }
            written = true;
        }
    }
    if (!written && t < T && a.dlogits != nullptr)
        for (int q = 0; q < Q; ++q) a.dlogits[col + (long)q * T] = 0.0f;
    if (a.pos_loss != nullptr && t < T) a.pos_loss[(long)b * T + t] = rl;
    const float trl = wave_reduce_sum(rl), tce = wave_reduce_sum(ce);
    amax = wc_wave_absmax(amax);
    if (lane == 0) {
        a.part[pidx] = trl;
        a.part[pn + pidx] = tce;
        if (a.dlogits != nullptr) a.part[2 * pn + pidx] = amax;
    }
}

// D = sum_i r_i w_{y_i} over the loss positions, first half: reads target and r only, a product per position in double (exact),
// one partial per workgroup of WC_DPOS positions; threads, lanes and waves are added in a fixed order.
__global__ __launch_bounds__(WC_TPB) void k_ce_divisor(const int64_t* __restrict__ target, const float* __restrict__ cw,
                                                       const float* __restrict__ r, const int* __restrict__ t_end, int T, int Q,
                                                       int t_start, double* __restrict__ dpart) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const int te = (t_end && t_end[b] < T) ? t_end[b] : T;
    double acc = 0.0;
    for (int j = 0; j < WC_DPOS / WC_TPB; ++j) {
        const int t = blockIdx.x * WC_DPOS + j * WC_TPB + (int)threadIdx.x;
        if (t >= t_start && t < te) {
            const long at = (long)b * T + t;
            const float wy = cw != nullptr ? cw[wc_class(target, at, Q)] : 1.0f;
            const float rr = r != nullptr ? r[at] : 1.0f;
            acc += (double)rr * (double)wy;
        }
    }
    acc = wn_wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dpart[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// second half, one workgroup: dw = {D, 1 / D}, the partials added in an order that depends on their number alone; D == 0
// (no weight on any loss position) leaves 1 / D = 0: the loss kernel then writes zeros
__global__ __launch_bounds__(WC_TPB) void k_ce_divisor_tail(const double* __restrict__ dpart, int n, double* __restrict__ dw) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += WC_TPB) acc += dpart[i];
    acc = wn_wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double D = (red[0] + red[1]) + (red[2] + red[3]);
    dw[0] = D;
    dw[1] = D > 0.0 ? 1.0 / D : 0.0;
}

// loss3 = {loss_scale sum r l / D, loss_scale sum ce / n_loss, D}: the partials added in double, each thread its strided share
// in ascending order, then lanes, then waves -- an order that depends on n alone.  One workgroup.
__global__ __launch_bounds__(WC_TPB) void k_cew_reduce(const float* __restrict__ part, int n, double loss_scale, double n_loss,
                                                       const double* __restrict__ dw, double d_host, int with_amax,
                                                       float* __restrict__ loss3, float* __restrict__ amax_out) {
    __shared__ double red[2][4];
    __shared__ float red_amax[4];
    double rl = 0.0, ce = 0.0;
    float am = 0.0f;
    for (int i = threadIdx.x; i < n; i += WC_TPB) {
        rl += (double)part[i];
        ce += (double)part[n + i];
        if (with_amax) am = wc_absmax(am, part[2 * n + i]);
    }
    rl = wn_wave_sum_f64(rl);
    ce = wn_wave_sum_f64(ce);
    am = wc_wave_absmax(am);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = rl;
        red[1][w] = ce;
        red_amax[w] = am;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    rl = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    ce = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double D = dw != nullptr ? dw[0] : d_host;
    loss3[0] = D > 0.0 ? (float)((rl * loss_scale) / D) : 0.0f;
    loss3[1] = (float)((ce * loss_scale) / n_loss);
    loss3[2] = (float)D;
    amax_out[0] = wc_absmax(wc_absmax(red_amax[0], red_amax[1]), wc_absmax(red_amax[2], red_amax[3]));
}

static inline int wc_blocks(int T) { return (T + WC_POS - 1) / WC_POS; }
static inline int wc_dblocks(int T) { return (T + WC_DPOS - 1) / WC_DPOS; }

// scratch: doubles {D, 1 / D, divisor partials [B][ceil(T / 1024)]}, then the floats [3][B][ceil(T / 64)]
long wn_cew_scratch_floats(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return 2L * (2 + (long)B * wc_dblocks(T)) + 3L * B * wc_blocks(T);
}

// WN_CEW_WIDE=1 in the environment sends every launch to the thread-per-position kernel (A/B knob of tools/ce_options_timing.py:
// the two shapes on the same sizes)
static inline bool cew_force_wide() {
    const char* e = getenv("WN_CEW_WIDE");
    return e && *e && atoi(e) != 0;
}

static int cew_divisor_launch(const WcArgs& a, int B, double* dw, wn_stream_t st) {
    const int nd = wc_dblocks(a.T);
    {
        WN_PROF("ce_divisor", 0.0, (8.0 + (a.r != nullptr ? 4.0 : 0.0)) * (double)B * (double)a.T, st);
        WN_LAUNCH(k_ce_divisor, dim3((unsigned)nd, (unsigned)B), dim3(WC_TPB), 0, st, a.target, a.cw, a.r, a.t_end, a.T, a.Q,
                  a.t_start, dw + 2);
    }
    WN_PROF("ce_divisor_tail", 0.0, 0.0, st);
    WN_LAUNCH(k_ce_divisor_tail, dim3(1), dim3(WC_TPB), 0, st, (const double*)(dw + 2), B * nd, dw);
    return 0;
}

static int cew_launch(const WcArgs& a, int B, wn_stream_t st) {
    // the bytes of the single-read shape: the logits once, dlogits once
    WN_PROF("softmax_cew", 0.0, (a.dlogits != nullptr ? 2.0 : 1.0) * 4.0 * (double)B * (double)a.Q * (double)a.T, st);
    const dim3 grid((unsigned)wc_blocks(a.T), (unsigned)B);
    // (the register-resident kernel addresses a wave's 64 rows as one buffer with 32-bit byte offsets)
    if (a.Q > 256 || (long)a.T * 256 >= 0x7ffffff0L || cew_force_wide()) {
        WN_LAUNCH(k_softmax_cew_wide, grid, dim3(WC_POS), 0, st, a);
    } else if (a.qw <= 16) {
        WN_LAUNCH(k_softmax_cew<16>, grid, dim3(WC_TPB), 0, st, a);
    } else if (a.qw <= 32) {
        WN_LAUNCH(k_softmax_cew<32>, grid, dim3(WC_TPB), 0, st, a);
    } else {
        WN_LAUNCH(k_softmax_cew<64>, grid, dim3(WC_TPB), 0, st, a);
    }
    return 0;
}

static int cew_reduce_launch(const float* part, int n, double loss_scale, double n_loss, const double* dw, double d_host,
                             int with_amax, float* loss3, float* amax_out, wn_stream_t st) {
    WN_PROF("cew_reduce", 0.0, 0.0, st);
    WN_LAUNCH(k_cew_reduce, dim3(1), dim3(WC_TPB), 0, st, part, n, loss_scale, n_loss, dw, d_host, with_amax, loss3, amax_out);
    return 0;
}

int wn_softmax_cew(const float* logits, const int64_t* target, const float* class_weights, const float* pos_weights, float* dlogits,
                   float* pos_loss, float* scratch, int B, int T, int Q, int t_start, const int* t_end, double n_loss, float eps,
                   int normalize, float grad_scale, float loss_scale, float* loss3, float* amax_out, wn_stream_t st) {
    if (B < 1 || T < 1 || Q < 1 || !(n_loss > 0.0) || ((uintptr_t)scratch & 7u) != 0) return 1;
    double* dw = (double*)scratch;
    // the divisor is on the device only where it depends on the data: "weights" with a weight of either kind
    const bool on_device = normalize == 0 && (class_weights != nullptr || pos_weights != nullptr);
    WcArgs a;
    a.s = logits; a.target = target; a.cw = class_weights; a.r = pos_weights; a.dlogits = dlogits; a.pos_loss = pos_loss;
    a.part = scratch + 2 * (2 + (long)B * wc_dblocks(T));
    a.t_end = t_end; a.dw = on_device ? dw : nullptr; a.inv_d = 1.0 / n_loss;
    a.T = T; a.Q = Q; a.t_start = t_start; a.qw = (Q + 3) / 4;
    a.eps = eps; a.gs = grad_scale;
    if (on_device && cew_divisor_launch(a, B, dw, st)) return 1;
    if (cew_launch(a, B, st)) return 1;
    return cew_reduce_launch(a.part, B * wc_blocks(T), (double)loss_scale, n_loss, a.dw, n_loss, dlogits != nullptr, loss3, amax_out, st);
}
