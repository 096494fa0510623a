// wn_sample.h -- temperature / top-k / nucleus (top-p) token choice of the decode kernels, written ONCE: one wave64 per
// utterance, called by k_decode (wn_decode.hip), k_dlp / k_dlpm / k_dlpf (the persistent any-size kernels) and
// k_dl_select_filtered (wn_elem.hip, the layer-wise launches).  Only the primitives of wn_device.h that the host emulator has too.
//
// Semantics, Q classes with raw logits l_q, one setting per call:
//   1. s_q = fp32(l_q * inv_t)                      one multiply that is never contracted into a neighbouring fma
//   2. top-k: v_k = the k-th largest s counted with multiplicity, A = {q : s_q >= v_k} (ties at v_k all kept; k = 0 or k >= Q: off)
//   3. top-p: e_q = expf(s_q - s_max); tau = the largest v among {s_q : q in A} with  sum_{q in A, s_q >= v} e_q >= p * sum_{q in A} e_q;
//      B = {q in A : s_q >= tau} (ties all kept, the maximal class is always in B; p >= 1: off)
//   4. the plain modes' inverse CDF restricted to B: in index order the first q in B whose running sum of e reaches u * total
//
// v_k and tau are found by bisection on the order-preserving integer image of the float keys (at most 32 steps each, every step
// one wave-reduced count / sum).  Both predicates are monotone in the threshold -- the count trivially, the fp32 sum because a
// fixed-order sum of non-negative terms rounded to nearest is monotone in each term -- so the bisection ends on a key that IS a
// class's value.  Reduction orders are fixed: a lane adds its own classes in ascending index order, lanes are combined by the
// xor butterfly 1, 2, 4, 8, 16, 32 (wn_xor_add); the draw's running sum is the plain modes' (inclusive scan over lanes).  A
// result depends on its inputs only, so every workgroup of a persistent launch that chooses for itself chooses the same token.
#pragma once
#include "wn_device.h"

#define WN_SAMPLE_NV 8                         // classes per lane
#define WN_SAMPLE_QMAX (64 * WN_SAMPLE_NV)     // most classes the filtered choice takes (the launchers refuse more)

// the per-call setting as the kernels take it (the host has validated it): top_k 0 = off, top_p >= 1 = off
struct WnSampleSet {
    float inv_t;
    int top_k;
    float top_p;
};

// a < b  <=>  key(a) < key(b) for all non-NaN floats; -0 and +0 share a key; no float maps to key 0 but a NaN
static __device__ __forceinline__ unsigned wn_sample_key(float s) {
    const unsigned u = wn_f32_bits(s);
    if ((u << 1) == 0u) return 0x80000000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

static __device__ __forceinline__ float wn_sample_wave_sum(float v) {
    v = wn_xor_add(v, 1);
    v = wn_xor_add(v, 2);
    v = wn_xor_add(v, 4);
    v = wn_xor_add(v, 8);
    v = wn_xor_add(v, 16);
    v = wn_xor_add(v, 32);
    return v;
}

// All 64 lanes of a wave call this with wave-uniform arguments (logit(q): the raw logit of class q < Q of the wave's utterance,
// Q <= WN_SAMPLE_QMAX); every lane returns the token.  Lane i holds the classes i * per .. i * per + per - 1, per = ceil(Q / 64).
template <class Logit>
static __device__ __forceinline__ int wn_sample_filtered(Logit logit, int Q, int lane, WnSampleSet f, float u) {
    const int per = (Q + 63) >> 6;
    const int q0 = lane * per;
    unsigned key[WN_SAMPLE_NV];   // 0: not a class / filtered out
    float e[WN_SAMPLE_NV];        // s, then expf(s - s_max), then 0 where filtered out
    float smax = -3.0e38f;
    WN_UNROLL
    for (int i = 0; i < WN_SAMPLE_NV; ++i) {
        const int q = q0 + i;
        const bool on = i < per && q < Q;
        e[i] = on ? wn_fmul_rn(logit(on ? q : 0), f.inv_t) : -3.0e38f;
        key[i] = on ? wn_sample_key(e[i]) : 0u;
        smax = fmaxf(smax, e[i]);
    }
    smax = wave_reduce_max(smax);
    const unsigned kmax = wn_sample_key(smax);
    int first = 0x7fffffff;       // first maximal class: the choice when no class reaches the target (a NaN draw), as in the plain modes
    WN_UNROLL
    for (int i = 0; i < WN_SAMPLE_NV; ++i) {
        if (key[i] == kmax && first == 0x7fffffff) first = q0 + i;
        e[i] = key[i] != 0u ? expf(e[i] - smax) : 0.0f;
    }
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_xor(first, m, 64);
        first = o < first ? o : first;
    }
    unsigned lo = 1u;             // every class passes key >= lo
    if (f.top_k > 0 && f.top_k < Q) {
        const float want = (float)f.top_k;   // counts up to 512 are exact in fp32: the float butterfly (DPP moves) counts them
        unsigned hi = kmax;
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo + 1u) >> 1);
            float c = 0.0f;
            WN_UNROLL
            for (int i = 0; i < WN_SAMPLE_NV; ++i) c += key[i] >= mid ? 1.0f : 0.0f;
            c = wn_sample_wave_sum(c);
            if (c >= want) lo = mid;
            else hi = mid - 1u;
        }
        WN_UNROLL
        for (int i = 0; i < WN_SAMPLE_NV; ++i)
            if (key[i] < lo) { key[i] = 0u; e[i] = 0.0f; }
    }
    if (f.top_p < 1.0f) {
        float all = 0.0f;
        WN_UNROLL
        for (int i = 0; i < WN_SAMPLE_NV; ++i) all += e[i];
        all = wn_sample_wave_sum(all);
        const float need = f.top_p * all;    // <= all: the whole of A passes, so lo does
        unsigned hi = kmax;
        while (lo < hi) {
            const unsigned mid = lo + ((hi - lo + 1u) >> 1);
            float c = 0.0f;
            WN_UNROLL
            for (int i = 0; i < WN_SAMPLE_NV; ++i) c += key[i] >= mid ? e[i] : 0.0f;
            c = wn_sample_wave_sum(c);
            if (c >= need) lo = mid;
            else hi = mid - 1u;
        }
        WN_UNROLL
        for (int i = 0; i < WN_SAMPLE_NV; ++i)
            if (key[i] < lo) { key[i] = 0u; e[i] = 0.0f; }
    }
    // inverse CDF over the classes that are left (the plain modes' scan: wn_decode.hip)
    float lsum = 0.0f;
    WN_UNROLL
    for (int i = 0; i < WN_SAMPLE_NV; ++i) lsum += e[i];
    float incl = lsum;
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl(incl, lane >= off ? lane - off : lane, 64);
        if (lane >= off) incl += o;
    }
    const float total = __shfl(incl, 63, 64);
    const float target = u * total;
    int cand = 0x7fffffff;
    float run = incl - lsum;
    WN_UNROLL
    for (int i = 0; i < WN_SAMPLE_NV; ++i) {
        run += e[i];
        if (cand == 0x7fffffff && key[i] != 0u && run >= target) cand = q0 + i;
    }
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_xor(cand, m, 64);
        cand = o < cand ? o : cand;
    }
    return cand != 0x7fffffff ? cand : first;
}
