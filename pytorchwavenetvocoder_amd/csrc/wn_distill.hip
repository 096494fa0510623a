// wn_distill.hip -- the soft-target loss head: hard-label cross-entropy blended with the tempered KL divergence from a
// teacher's logits (knowledge distillation, Hinton's form), and its gradient with respect to the student's logits (gfx950).
//
// A streaming kernel: student logits in, teacher logits in, dlogits out.  One thread per position with two passes over the
// column (k_softmax_ce's shape) would read both inputs twice, so for Q <= 256 a workgroup of 4 waves covers 64 consecutive
// positions and wave w keeps the classes [w * ceil(Q / 4), ..) of those positions in registers -- at most 64 student and 64
// teacher values per lane.  The column maxima, the exponential sums and the kl numerator cross the 4 waves through LDS, and
// dlogits is written from the registers.  Every global access is 64 consecutive t per instruction (256 B).
//
// Arithmetic (wn_elem.hip, k_softmax_ce): the column maximum is subtracted before the division by tau, (v - max) / tau, and
// log-probabilities are differences (v - max) / tau - log(sum), never formed through lse = log(sum) + max, which a common
// offset or a peak of some tens of nats would round at ulp(max).  With P = eu / Zu and log P - log S = (bu - bs) - log Zu + log Zs:
//   kl = (sum_q eu_q (bu_q - bs_q)) / Zu + log(Zs / Zu),   eu_q = exp(bu_q), a class with eu_q == 0 adds exactly 0,
// not clamped.  tau == 1: the student's tempered softmax is its plain one, one exponential per class.
#include "wn_distill.h"
#include "wn_prof.h"

#include <math.h>
#include <stdlib.h>

#define WD_POS 64    // positions per workgroup (one per lane)
#define WD_TPB 256   // 4 waves: a quarter of the classes each

// max(a, |v|) on the bit patterns: inf and NaN stay on top (the fp16 pair split of the backward pass then takes its redo)
static __device__ __forceinline__ float wd_absmax(float a, float v) {
    const int ai = __builtin_bit_cast(int, a), vi = __builtin_bit_cast(int, v) & 0x7fffffff;
    return __builtin_bit_cast(float, vi > ai ? vi : ai);
}
static __device__ __forceinline__ float wd_wave_absmax(float a) {
    int ai = __builtin_bit_cast(int, a);
    WN_UNROLL
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(ai, m, 64); ai = o > ai ? o : ai; }
    return __builtin_bit_cast(float, ai);
}

struct WdArgs {
    const float* s;       // student logits (B, Q, T)
    const float* u;       // teacher logits (B, Q, T)
    const int64_t* target;  // (B, T) or NULL (alpha == 1)
    float* dlogits;       // (B, Q, T) or NULL
    float* pos_loss;      // (B, T) or NULL
    float* part;          // [3][B][nblk]: ce sums, kl sums, max |dlogits|
    const int* t_end;     // (B) or NULL
    int T, Q, t_start, qw;  // qw = ceil(Q / 4): classes per wave
    float alpha, tau, gs;
};

// ce, kl and l of one position from the column sums.  Z1 = sum exp(s - ms), Zs = sum exp((s - ms) / tau), Zu likewise for the
// teacher, num = sum eu (bu - bs); sy = the target's logit (unused with alpha == 1)
static __device__ __forceinline__ void wd_position(const WdArgs& a, float ms, float sy, float Z1, float Zs, float Zu, float num,
                                                   float* ce, float* kl, float* l) {
    *ce = a.alpha == 1.0f ? 0.0f : (ms - sy) + logf(Z1);
    // log Zs - log Zu as ONE logarithm of a ratio in [1 / Q, Q]: two logarithms of some nats each would round at their own
    // magnitude, which is what is left of a small kl after the difference
    *kl = num / Zu + logf(Zs / Zu);
    *l = a.alpha == 0.0f ? *ce : (a.alpha == 1.0f ? (a.tau * a.tau) * *kl : (1.0f - a.alpha) * *ce + (a.alpha * a.tau * a.tau) * *kl);
}

template <int NQ>
__global__ __launch_bounds__(WD_TPB) void k_softmax_distill(const WdArgs a) {
    __shared__ float red_max[2][4][WD_POS];
    __shared__ float red_sum[4][4][WD_POS];
    __shared__ float red_amax[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.y, T = a.T, Q = a.Q;
    const int t0 = blockIdx.x * WD_POS, t = t0 + lane;
    const int te = (a.t_end && a.t_end[b] < T) ? a.t_end[b] : T;   // ragged batch: the sequence's own end (block-uniform)
    const bool live = t >= a.t_start && t < te;
    const int q0 = w * a.qw;
    const int qn = Q - q0 < a.qw ? (Q - q0 < 0 ? 0 : Q - q0) : a.qw;   // classes of this wave (wave-uniform)
    // buffer access (wn_device.h): the wave's rows are one buffer of qn * T floats, a row is a wave-uniform offset and the
    // position the only per-lane address register; lanes that must not read or write carry an offset past the buffer
    const long row0 = ((long)b * Q + q0) * T;
    const unsigned rows_bytes = (unsigned)qn * (unsigned)T * 4u;
    const wn_rsrc_t bs_ = wn_make_buf(a.s + row0, rows_bytes), bu_ = wn_make_buf(a.u + row0, rows_bytes);
    const wn_rsrc_t bd_ = wn_make_buf(a.dlogits != nullptr ? a.dlogits + row0 : a.s, a.dlogits != nullptr ? rows_bytes : 0u);
    const int v_ld = live ? t * 4 : WN_VOFF_DEAD, v_st = t < T ? t * 4 : WN_VOFF_DEAD;
    const int row_bytes = T * 4;
    const int pidx = blockIdx.y * gridDim.x + blockIdx.x, pn = gridDim.x * gridDim.y;
    if (t0 + WD_POS <= a.t_start || t0 >= te) {   // no live position in the block: zeros out, no logit read
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
    // the wave's quarter of both columns, read once; slots past the wave's classes hold -inf (exp -> 0), dead positions read
    // nothing (their lanes compute on zeros and contribute nowhere)
    float s[NQ], u[NQ];
    WN_UNROLL
    for (int i = 0; i < NQ; ++i) {
        s[i] = i < qn ? wn_buf_load_once(bs_, v_ld, i * row_bytes) : -INFINITY;
        u[i] = i < qn ? wn_buf_load_once(bu_, v_ld, i * row_bytes) : -INFINITY;
    }
    float ms = -INFINITY, mu = -INFINITY;
    WN_UNROLL
    for (int i = 0; i < NQ; ++i) {
        ms = fmaxf(ms, s[i]);
        mu = fmaxf(mu, u[i]);
    }
    red_max[0][w][lane] = ms;
    red_max[1][w][lane] = mu;
    __syncthreads();
    ms = fmaxf(fmaxf(red_max[0][0][lane], red_max[0][1][lane]), fmaxf(red_max[0][2][lane], red_max[0][3][lane]));
    mu = fmaxf(fmaxf(red_max[1][0][lane], red_max[1][1][lane]), fmaxf(red_max[1][2][lane], red_max[1][3][lane]));
    const bool tau1 = a.tau == 1.0f;   // (uniform)
    // four interleaved accumulators per sum, added as a tree: a chain of 16 terms at most, not of 64
    float Z1a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Zsa[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Zua[4] = {0.0f, 0.0f, 0.0f, 0.0f},
          numa[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (tau1) {
        WN_UNROLL
        for (int i = 0; i < NQ; ++i) {
            if (i < qn) {
                const float as = s[i] - ms, bu = u[i] - mu;
                const float es = expf(as), eu = expf(bu);
                Z1a[i & 3] += es;
                Zua[i & 3] += eu;
                if (eu > 0.0f) numa[i & 3] += eu * (bu - as);
                s[i] = es;   // softmax numerators from here on
                u[i] = eu;
            }
        }
    } else {
        WN_UNROLL
        for (int i = 0; i < NQ; ++i) {
            if (i < qn) {
                const float as = s[i] - ms;
                const float bs = as / a.tau, bu = (u[i] - mu) / a.tau;
                const float eu = expf(bu);
                Z1a[i & 3] += expf(as);
                Zsa[i & 3] += expf(bs);
                Zua[i & 3] += eu;
                if (eu > 0.0f) numa[i & 3] += eu * (bu - bs);
                s[i] = as;   // the student keeps s - max: two softmaxes are formed from it
                u[i] = eu;
            }
        }
    }
    float Z1 = (Z1a[0] + Z1a[1]) + (Z1a[2] + Z1a[3]), Zu = (Zua[0] + Zua[1]) + (Zua[2] + Zua[3]);
    float Zs = tau1 ? Z1 : (Zsa[0] + Zsa[1]) + (Zsa[2] + Zsa[3]), num = (numa[0] + numa[1]) + (numa[2] + numa[3]);
    red_sum[0][w][lane] = Z1;
    red_sum[1][w][lane] = Zs;
    red_sum[2][w][lane] = Zu;
    red_sum[3][w][lane] = num;
    __syncthreads();
    Z1 = (red_sum[0][0][lane] + red_sum[0][1][lane]) + (red_sum[0][2][lane] + red_sum[0][3][lane]);
    Zs = (red_sum[1][0][lane] + red_sum[1][1][lane]) + (red_sum[1][2][lane] + red_sum[1][3][lane]);
    Zu = (red_sum[2][0][lane] + red_sum[2][1][lane]) + (red_sum[2][2][lane] + red_sum[2][3][lane]);
    num = (red_sum[3][0][lane] + red_sum[3][1][lane]) + (red_sum[3][2][lane] + red_sum[3][3][lane]);
    // class index modulo Q like k_softmax_ce; alpha == 1 reads no target
    int y = -1;
    if (live && a.alpha != 1.0f) {
        long long tg = a.target[(long)b * T + t] % Q;
        if (tg < 0) tg += Q;
        y = (int)tg;
    }
    if (w == 0) {
        float ce = 0.0f, kl = 0.0f, l = 0.0f;
        if (live) {
            const float sy = y >= 0 ? a.s[((long)b * Q + y) * T + t] : 0.0f;
            wd_position(a, ms, sy, Z1, Zs, Zu, num, &ce, &kl, &l);
        }
        if (a.pos_loss != nullptr && t < T) a.pos_loss[(long)b * T + t] = l;
        const float tce = wave_reduce_sum(ce), tkl = wave_reduce_sum(kl);
        if (lane == 0) {
            a.part[pidx] = tce;
            a.part[pn + pidx] = tkl;
        }
    }
    if (a.dlogits == nullptr) return;
    float amax = 0.0f;
    if (live) {
        const float r1 = 1.0f / Z1, rs = 1.0f / Zs, ru = 1.0f / Zu;
        const float c1 = 1.0f - a.alpha, c2 = a.alpha * a.tau;
        const int yl = y - q0;
        WN_UNROLL
        for (int i = 0; i < NQ; ++i) {
            if (i < qn) {
                float p1, S;
                if (tau1) {
                    p1 = s[i] * r1;
                    S = p1;
                } else {
                    p1 = expf(s[i]) * r1;
                    S = expf(s[i] / a.tau) * rs;
                }
                const float P = u[i] * ru;
                const float d = (c1 * (p1 - (i == yl ? 1.0f : 0.0f)) + c2 * (S - P)) * a.gs;
                wn_buf_store(bd_, d, v_st, i * row_bytes);
                amax = wd_absmax(amax, d);
            }
        }
    } else {
        for (int i = 0; i < qn; ++i) wn_buf_store(bd_, 0.0f, v_st, i * row_bytes);
    }
    amax = wd_wave_absmax(amax);
    if (lane == 0) red_amax[w] = amax;
    __syncthreads();
    if (threadIdx.x == 0) a.part[2 * pn + pidx] = wd_absmax(wd_absmax(red_amax[0], red_amax[1]), wd_absmax(red_amax[2], red_amax[3]));
}

// More than 256 classes: one thread per position, plain loops over the column (three reads of each input).  Same partials.
__global__ __launch_bounds__(WD_POS) void k_softmax_distill_wide(const WdArgs a) {
    const int lane = threadIdx.x;
    const int b = blockIdx.y, T = a.T, Q = a.Q;
    const int t = blockIdx.x * WD_POS + lane;
    const int te = (a.t_end && a.t_end[b] < T) ? a.t_end[b] : T;
    const bool live = t >= a.t_start && t < te;
    const long col = (long)b * Q * T + t;
    const int pidx = blockIdx.y * gridDim.x + blockIdx.x, pn = gridDim.x * gridDim.y;
    float ce = 0.0f, kl = 0.0f, l = 0.0f, amax = 0.0f;
    if (live) {
        const float* sp = a.s + col;
        const float* up = a.u + col;
        float ms = -INFINITY, mu = -INFINITY;
        for (int q = 0; q < Q; ++q) {
            ms = fmaxf(ms, sp[(long)q * T]);
            mu = fmaxf(mu, up[(long)q * T]);
        }
        const bool tau1 = a.tau == 1.0f;
        // eight interleaved accumulators per sum, added as a tree (the chains stay short: the sums' rounding, not their terms',
        // would otherwise set the error of kl)
        float Z1a[8], Zsa[8], Zua[8], numa[8];
        for (int k = 0; k < 8; ++k) Z1a[k] = Zsa[k] = Zua[k] = numa[k] = 0.0f;
        for (int q = 0; q < Q; ++q) {
            const float as = sp[(long)q * T] - ms;
            const float bs = tau1 ? as : as / a.tau;
            const float bu = tau1 ? up[(long)q * T] - mu : (up[(long)q * T] - mu) / a.tau;
            const float es = expf(as), eu = expf(bu);
            Z1a[q & 7] += es;
            Zsa[q & 7] += tau1 ? es : expf(bs);
            Zua[q & 7] += eu;
            if (eu > 0.0f) numa[q & 7] += eu * (bu - bs);
        }
        const float Z1 = ((Z1a[0] + Z1a[1]) + (Z1a[2] + Z1a[3])) + ((Z1a[4] + Z1a[5]) + (Z1a[6] + Z1a[7]));
        const float Zs = ((Zsa[0] + Zsa[1]) + (Zsa[2] + Zsa[3])) + ((Zsa[4] + Zsa[5]) + (Zsa[6] + Zsa[7]));
        const float Zu = ((Zua[0] + Zua[1]) + (Zua[2] + Zua[3])) + ((Zua[4] + Zua[5]) + (Zua[6] + Zua[7]));
        const float num = ((numa[0] + numa[1]) + (numa[2] + numa[3])) + ((numa[4] + numa[5]) + (numa[6] + numa[7]));
        int y = -1;
        float sy = 0.0f;
        if (a.alpha != 1.0f) {
            long long tg = a.target[(long)b * T + t] % Q;
            if (tg < 0) tg += Q;
            y = (int)tg;
            sy = sp[(long)y * T];
        }
        wd_position(a, ms, sy, Z1, Zs, Zu, num, &ce, &kl, &l);
        if (a.dlogits != nullptr) {
            const float r1 = 1.0f / Z1, rs = 1.0f / Zs, ru = 1.0f / Zu;
            const float c1 = 1.0f - a.alpha, c2 = a.alpha * a.tau;
            for (int q = 0; q < Q; ++q) {
                const float as = sp[(long)q * T] - ms;
                const float p1 = expf(as) * r1;
                const float S = tau1 ? p1 : expf(as / a.tau) * rs;
                const float P = expf(tau1 ? up[(long)q * T] - mu : (up[(long)q * T] - mu) / a.tau) * ru;
                const float d = (c1 * (p1 - (q == y ? 1.0f : 0.0f)) + c2 * (S - P)) * a.gs;
                a.dlogits[col + (long)q * T] = d;
                amax = wd_absmax(amax, d);
            }
        }
    } else if (t < T && a.dlogits != nullptr) {
        for (int q = 0; q < Q; ++q) a.dlogits[col + (long)q * T] = 0.0f;
    }
    if (a.pos_loss != nullptr && t < T) a.pos_loss[(long)b * T + t] = l;
    const float tce = wave_reduce_sum(ce), tkl = wave_reduce_sum(kl);
    amax = wd_wave_absmax(amax);
    if (lane == 0) {
        a.part[pidx] = tce;
        a.part[pn + pidx] = tkl;
        if (a.dlogits != nullptr) a.part[2 * pn + pidx] = amax;
    }
}

// loss3 = scale * {(1 - alpha) sum ce + alpha tau^2 sum kl, sum ce, sum kl}: the partials added in double, each thread its
// strided share in ascending order, then lanes, then waves -- an order that depends on n alone.  One workgroup.
__global__ __launch_bounds__(WD_TPB) void k_distill_reduce(const float* __restrict__ part, int n, float scale, float alpha, float tau,
                                                           int with_amax, float* __restrict__ loss3, float* __restrict__ amax_out) {
    __shared__ double red[2][4];
    __shared__ float red_amax[4];
    double ce = 0.0, kl = 0.0;
    float am = 0.0f;
    for (int i = threadIdx.x; i < n; i += WD_TPB) {
        ce += (double)part[i];
        kl += (double)part[n + i];
        if (with_amax) am = wd_absmax(am, part[2 * n + i]);
    }
    ce = wn_wave_sum_f64(ce);
    kl = wn_wave_sum_f64(kl);
    am = wd_wave_absmax(am);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w] = ce;
        red[1][w] = kl;
        red_amax[w] = am;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    ce = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    kl = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double wkl = (double)alpha * (double)tau * (double)tau, wce = 1.0 - (double)alpha;
    const double tot = alpha == 0.0f ? ce : (alpha == 1.0f ? wkl * kl : wce * ce + wkl * kl);
    loss3[0] = (float)(tot * (double)scale);
    loss3[1] = (float)(ce * (double)scale);
    loss3[2] = (float)(kl * (double)scale);
    amax_out[0] = wd_absmax(wd_absmax(red_amax[0], red_amax[1]), wd_absmax(red_amax[2], red_amax[3]));
}

long wn_distill_scratch_floats(int B, int T) {
    if (B < 1 || T < 1) return 0;
    return 3L * B * ((T + WD_POS - 1) / WD_POS);
}

// WN_DISTILL_WIDE=1 in the environment sends every launch to the thread-per-position kernel (A/B knob of tools/distill_timing.py:
// the two shapes on the same sizes)
static inline bool distill_force_wide() {
    const char* e = getenv("WN_DISTILL_WIDE");
    return e && *e && atoi(e) != 0;
}

static int distill_launch(const WdArgs& a, int B, wn_stream_t st) {
    // the bytes of the single-read shape: both inputs once, dlogits once
    WN_PROF("softmax_distill", 0.0, (a.dlogits != nullptr ? 3.0 : 2.0) * 4.0 * (double)B * (double)a.Q * (double)a.T, st);
    const dim3 grid((unsigned)((a.T + WD_POS - 1) / WD_POS), (unsigned)B);
    // (the register-resident kernel addresses a wave's 64 rows as one buffer with 32-bit byte offsets)
    if (a.Q > 256 || (long)a.T * 256 >= 0x7ffffff0L || distill_force_wide()) {
        WN_LAUNCH(k_softmax_distill_wide, grid, dim3(WD_POS), 0, st, a);
    } else if (a.qw <= 16) {
        WN_LAUNCH(k_softmax_distill<16>, grid, dim3(WD_TPB), 0, st, a);
    } else if (a.qw <= 32) {
        WN_LAUNCH(k_softmax_distill<32>, grid, dim3(WD_TPB), 0, st, a);
    } else {
        WN_LAUNCH(k_softmax_distill<64>, grid, dim3(WD_TPB), 0, st, a);
    }
    return 0;
}

static int distill_reduce_launch(const float* part, int n, float scale, float alpha, float tau, int with_amax, float* loss3,
                                 float* amax_out, wn_stream_t st) {
    WN_PROF("distill_reduce", 0.0, 0.0, st);
    WN_LAUNCH(k_distill_reduce, dim3(1), dim3(WD_TPB), 0, st, part, n, scale, alpha, tau, with_amax, loss3, amax_out);
    return 0;
}

int wn_softmax_distill(const float* logits, const float* teacher, const int64_t* target, float* dlogits, float* pos_loss,
                       float* scratch, int B, int T, int Q, int t_start, const int* t_end, float alpha, float tau, float gs,
                       float scale, float* loss3, float* amax_out, wn_stream_t st) {
    if (B < 1 || T < 1 || Q < 1) return 1;
    WdArgs a;
    a.s = logits; a.u = teacher; a.target = target; a.dlogits = dlogits; a.pos_loss = pos_loss; a.part = scratch; a.t_end = t_end;
    a.T = T; a.Q = Q; a.t_start = t_start; a.qw = (Q + 3) / 4;
    a.alpha = alpha; a.tau = tau; a.gs = gs;
    if (distill_launch(a, B, st)) return 1;
    const int n = B * ((T + WD_POS - 1) / WD_POS);
    return distill_reduce_launch(scratch, n, scale, alpha, tau, dlogits != nullptr, loss3, amax_out, st);
}
