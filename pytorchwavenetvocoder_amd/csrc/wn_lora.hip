// wn_lora.hip -- low-rank adapters W = W0 + scale B A over the flat buffers (wn_lora.h).
//
// Both operations walk the same list of 64 x 64 tiles of the adapted matrices, one workgroup per tile:
//   k_lora_merge     stages the tile's 64 columns of A and 64 rows of B in LDS and writes params = fmaf(scale, sum_k B A, base)
//                    for the tile's elements, k ascending.  Elements outside every entry are never addressed.
//   k_lora_partials  stages the tile of g once, beside the same pieces of A and B, and forms the tile's share of
//                    dA[k, c] = sum_o B[o, k] g[o, c] (rows of the tile ascending) and of dB[o, k] = sum_c g[o, c] A[k, c]
//                    (columns of the tile ascending): g is read from memory once.
//   k_lora_reduce    sums the shares in tile order and multiplies by scale: no atomics, every order fixed by the table.
// Matrices sit at arbitrary 4-byte aligned offsets and their rows need not be multiples of four elements, so every row segment
// of a tile splits into a scalar head, 16-byte quads and a scalar tail by its own address (wn_lora_seg); a pair of buffers whose
// addresses differ modulo 16 goes scalar altogether.  An element gets the same expression on every path.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "wn_lora.h"
#include "wn_prof.h"

#define WN_LORA_LD (WN_LORA_TILE + 1)   // LDS row stride: odd, so a column walk meets every bank once

struct WnLoraTile {
    long w_off, rows, cols, a_off, b_off, scratch_off;
    int rank, r0, c0, nr, nc, rt, ct, n_rt, n_ct;
    float scale;
};

static __device__ __forceinline__ WnLoraTile wn_lora_tile(const long* __restrict__ T, long word) {
    const long* e = T + WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * (word >> 32);
    const long tile = word & 0xffffffffL;
    WnLoraTile t;
    t.w_off = e[0], t.rows = e[1], t.cols = e[2], t.rank = (int)e[3], t.a_off = e[4], t.b_off = e[5];
    t.scale = wn_bits_f32((unsigned)e[6]);
    t.scratch_off = e[7];
    t.n_rt = (int)((t.rows + WN_LORA_TILE - 1) / WN_LORA_TILE);
    t.n_ct = (int)((t.cols + WN_LORA_TILE - 1) / WN_LORA_TILE);
    t.rt = (int)(tile / t.n_ct), t.ct = (int)(tile % t.n_ct);
    t.r0 = t.rt * WN_LORA_TILE, t.c0 = t.ct * WN_LORA_TILE;
    t.nr = (int)(t.rows - t.r0 < WN_LORA_TILE ? t.rows - t.r0 : WN_LORA_TILE);
    t.nc = (int)(t.cols - t.c0 < WN_LORA_TILE ? t.cols - t.c0 : WN_LORA_TILE);
    return t;
}

// the tile's pieces of the factors: As[k][c] = A[k, c0 + c], Bs[o][k] = B[r0 + o, k]
static __device__ __forceinline__ void wn_lora_stage_factors(const WnLoraTile& t, const float* __restrict__ adapter,
                                                             float (*As)[WN_LORA_LD], float (*Bs)[WN_LORA_LD]) {
    for (int i = threadIdx.x; i < t.rank * WN_LORA_TILE; i += WN_LORA_TPB) {
        const int k = i >> 6, c = i & (WN_LORA_TILE - 1);
        if (c < t.nc) As[k][c] = adapter[t.a_off + (long)k * t.cols + t.c0 + c];
    }
    const float* b = adapter + t.b_off + (long)t.r0 * t.rank;   // the tile's rows of B are one contiguous run
    for (int i = threadIdx.x; i < t.nr * t.rank; i += WN_LORA_TPB) Bs[i / t.rank][i % t.rank] = b[i];
}

// The same for k_lora_partials<NK>, whose waves each walk NK ranks without a test: ranks up to KPAD = 4 NK and the rows and columns
// beyond the tile's edge are filled with zeros (what they contribute is never stored)
template <int KPAD>
static __device__ __forceinline__ void wn_lora_stage_factors_padded(const WnLoraTile& t, const float* __restrict__ adapter,
                                                                    float (*As)[WN_LORA_LD], float (*Bs)[WN_LORA_LD]) {
    for (int i = threadIdx.x; i < KPAD * WN_LORA_TILE; i += WN_LORA_TPB) {
        const int k = i >> 6, c = i & (WN_LORA_TILE - 1);
        As[k][c] = (k < t.rank && c < t.nc) ? adapter[t.a_off + (long)k * t.cols + t.c0 + c] : 0.0f;
    }
    const float* b = adapter + t.b_off + (long)t.r0 * t.rank;
    for (int i = threadIdx.x; i < WN_LORA_TILE * KPAD; i += WN_LORA_TPB) {
        const int o = i / KPAD, k = i % KPAD;
        Bs[o][k] = (o < t.nr && k < t.rank) ? b[o * t.rank + k] : 0.0f;
    }
}

// A row segment of `len` <= 64 elements at p, walked by 16 threads (q = 0 .. 15): `head` scalar elements up to the first 16-byte
// boundary, `nq` quads, then a scalar tail.  aligned == false: no quads at all.
struct WnLoraSeg {
    int head, nq;
};
static __device__ __forceinline__ WnLoraSeg wn_lora_seg(const float* p, int len, bool aligned) {
    if (!aligned) return {len, 0};
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
    if (head > len) head = len;
    return {head, (len - head) >> 2};
}

__global__ __launch_bounds__(WN_LORA_TPB) void k_lora_merge(const float* __restrict__ base, float* __restrict__ params,
                                                            const float* __restrict__ adapter, const long* __restrict__ T) {
    __shared__ float As[WN_LORA_MAX_RANK][WN_LORA_LD];
    __shared__ float Bs[WN_LORA_TILE][WN_LORA_LD];
    const WnLoraTile t = wn_lora_tile(T, T[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * T[1] + blockIdx.x]);
    wn_lora_stage_factors(t, adapter, As, Bs);
    __syncthreads();
    const bool aligned = (reinterpret_cast<uintptr_t>(base) & 15) == (reinterpret_cast<uintptr_t>(params) & 15);
    const int q = threadIdx.x & 15;
    auto delta = [&](int o, int c) {
        float acc = 0.0f;
        for (int k = 0; k < t.rank; ++k) acc = fmaf(Bs[o][k], As[k][c], acc);
        return acc;
    };
    for (int o = threadIdx.x >> 4; o < t.nr; o += WN_LORA_TPB >> 4) {
        const long i0 = t.w_off + (long)(t.r0 + o) * t.cols + t.c0;
        const WnLoraSeg s = wn_lora_seg(params + i0, t.nc, aligned);
        if (q < s.nq) {
            const int c = s.head + 4 * q;
            float4 v = *reinterpret_cast<const float4*>(base + i0 + c);
            v.x = fmaf(t.scale, delta(o, c), v.x);
            v.y = fmaf(t.scale, delta(o, c + 1), v.y);
            v.z = fmaf(t.scale, delta(o, c + 2), v.z);
            v.w = fmaf(t.scale, delta(o, c + 3), v.w);
            *reinterpret_cast<float4*>(params + i0 + c) = v;
        }
        for (int c = q; c < s.head; c += 16) params[i0 + c] = fmaf(t.scale, delta(o, c), base[i0 + c]);
        for (int c = s.head + 4 * s.nq + q; c < t.nc; c += 16) params[i0 + c] = fmaf(t.scale, delta(o, c), base[i0 + c]);
    }
}

// NK: accumulators per thread, 4 NK >= the largest rank of the table (the launcher picks the smallest of 1, 2, 4, 8, 16)
template <int NK>
__global__ __launch_bounds__(WN_LORA_TPB) void k_lora_partials(const float* __restrict__ g, const float* __restrict__ adapter,
                                                               const long* __restrict__ T, float* __restrict__ scratch) {
    __shared__ float As[WN_LORA_MAX_RANK][WN_LORA_LD];
    __shared__ float Bs[WN_LORA_TILE][WN_LORA_LD];
    __shared__ float Gs[WN_LORA_TILE][WN_LORA_LD];
    const WnLoraTile t = wn_lora_tile(T, T[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * T[1] + blockIdx.x]);
    wn_lora_stage_factors_padded<4 * NK>(t, adapter, As, Bs);
    {
        const int q = threadIdx.x & 15;
        for (int o = threadIdx.x >> 4; o < t.nr; o += WN_LORA_TPB >> 4) {
            const float* p = g + t.w_off + (long)(t.r0 + o) * t.cols + t.c0;
            const WnLoraSeg s = wn_lora_seg(p, t.nc, true);
            if (q < s.nq) {
                const int c = s.head + 4 * q;
                const float4 v = *reinterpret_cast<const float4*>(p + c);
                Gs[o][c] = v.x, Gs[o][c + 1] = v.y, Gs[o][c + 2] = v.z, Gs[o][c + 3] = v.w;
            }
            for (int c = q; c < s.head; c += 16) Gs[o][c] = p[c];
            for (int c = s.head + 4 * s.nq + q; c < t.nc; c += 16) Gs[o][c] = p[c];
        }
    }
    __syncthreads();
    // a wave takes the ranks k = wave, wave + 4, ...: the factor it multiplies by is one LDS broadcast, the tile of g is read
    // along a row (dA: lanes are columns) or down a column of odd stride (dB: lanes are rows)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the tile's share of dA, rows ascending: [n_rt][rank][cols]
    if (lane < t.nc) {
        float acc[NK];
        WN_UNROLL
        for (int j = 0; j < NK; ++j) acc[j] = 0.0f;
        WN_UNROLL_N(4)
        for (int o = 0; o < t.nr; ++o) {
            const float x = Gs[o][lane];
            WN_UNROLL
            for (int j = 0; j < NK; ++j) acc[j] = fmaf(Bs[o][wave + 4 * j], x, acc[j]);
        }
        float* pa = scratch + t.scratch_off + (long)t.rt * t.rank * t.cols + t.c0 + lane;
        WN_UNROLL
        for (int j = 0; j < NK; ++j)
            if (wave + 4 * j < t.rank) pa[(long)(wave + 4 * j) * t.cols] = acc[j];
    }
    // the tile's share of dB, columns ascending: [n_ct][rank][rows] behind the shares of dA
    if (lane < t.nr) {
        float acc[NK];
        WN_UNROLL
        for (int j = 0; j < NK; ++j) acc[j] = 0.0f;
        WN_UNROLL_N(4)
        for (int c = 0; c < t.nc; ++c) {
            const float x = Gs[lane][c];
            WN_UNROLL
            for (int j = 0; j < NK; ++j) acc[j] = fmaf(x, As[wave + 4 * j][c], acc[j]);
        }
        float* pb = scratch + t.scratch_off + (long)t.n_rt * t.rank * t.cols + (long)t.ct * t.rank * t.rows + t.r0 + lane;
        WN_UNROLL
        for (int j = 0; j < NK; ++j)
            if (wave + 4 * j < t.rank) pb[(long)(wave + 4 * j) * t.rows] = acc[j];
    }
}

__global__ __launch_bounds__(WN_LORA_TPB) void k_lora_reduce(const float* __restrict__ scratch, const long* __restrict__ T,
                                                             float* __restrict__ adapter_grads) {
    const long word = T[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * T[1] + T[2] + blockIdx.x];
    const WnLoraTile t = wn_lora_tile(T, word & ~0xffffffffL);
    const long i = (word & 0xffffffffL) * WN_LORA_TPB + threadIdx.x;
    const long n_a = (long)t.rank * t.cols, n_b = t.rows * t.rank;
    if (i >= n_a + n_b) return;
    const float* p;
    long stride, out;
    int n;
    if (i < n_a) {   // dA[k, c]: the shares of the row tiles, top to bottom
        p = scratch + t.scratch_off + i;
        stride = n_a, n = t.n_rt, out = t.a_off + i;
    } else {         // dB[o, k]: the shares of the column tiles, left to right
        const long o = (i - n_a) / t.rank, k = (i - n_a) % t.rank;
        p = scratch + t.scratch_off + (long)t.n_rt * n_a + k * t.rows + o;
        stride = n_b, n = t.n_ct, out = t.b_off + (i - n_a);
    }
    float acc = p[0];
    for (int b = 1; b < n; ++b) acc += p[b * stride];
    adapter_grads[out] = wn_fmul_rn(t.scale, acc);
}

// ---------------------------------------------------------------------------------------------
// host side
static int64_t lora_fail(char* err, size_t err_len, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    if (err && err_len) snprintf(err, err_len, fmt, a, b, c);
    return -1;
}

int64_t wn_lora_build_table(const struct WnLoraEntry* entries, int n_entries, int64_t n_model, int64_t n_adapter, int64_t* table,
                            int64_t table_words, char* err, size_t err_len) {
    if (!entries) return lora_fail(err, err_len, "wn_lora_table: entries is NULL");
    if (n_entries <= 0) return lora_fail(err, err_len, "wn_lora_table: an empty table (n_entries = %lld)", n_entries);
    if (n_model <= 0 || n_adapter <= 0) return lora_fail(err, err_len, "wn_lora_table: n_model <= 0 or n_adapter <= 0");
    struct Range {
        int64_t lo, hi;
        int entry;
    };
    std::vector<Range> model, adapter;
    int64_t tiles = 0, reduce = 0, scratch = 0;
    for (int e = 0; e < n_entries; ++e) {
        const WnLoraEntry& x = entries[e];
        if (x.rows < 1 || x.cols < 1 || x.rows > 0x7fffffff || x.cols > 0x7fffffff)
            return lora_fail(err, err_len, "wn_lora_table: entry %lld has rows = %lld, cols = %lld", e, x.rows, x.cols);
        if (x.rank < 1 || x.rank > WN_LORA_MAX_RANK)
            return lora_fail(err, err_len, "wn_lora_table: entry %lld has rank %lld outside [1, %lld]", e, x.rank, WN_LORA_MAX_RANK);
        if (x.rank > (x.rows < x.cols ? x.rows : x.cols))
            return lora_fail(err, err_len, "wn_lora_table: entry %lld has rank %lld above min(rows, cols) = %lld", e, x.rank,
                             x.rows < x.cols ? x.rows : x.cols);
        if (!std::isfinite(x.scale) || !std::isfinite((float)x.scale))
            return lora_fail(err, err_len, "wn_lora_table: entry %lld has a scale that is not finite", e);
        if (x.w_off < 0 || x.rows * x.cols > n_model - x.w_off)
            return lora_fail(err, err_len, "wn_lora_table: entry %lld: W at %lld lies outside the model buffer of %lld elements", e,
                             x.w_off, n_model);
        if (x.a_off < 0 || x.rank * x.cols > n_adapter - x.a_off)
            return lora_fail(err, err_len, "wn_lora_table: entry %lld: A at %lld lies outside the adapter buffer of %lld elements", e,
                             x.a_off, n_adapter);
        if (x.b_off < 0 || x.rows * x.rank > n_adapter - x.b_off)
            return lora_fail(err, err_len, "wn_lora_table: entry %lld: B at %lld lies outside the adapter buffer of %lld elements", e,
                             x.b_off, n_adapter);
        model.push_back({x.w_off, x.w_off + x.rows * x.cols, e});
        adapter.push_back({x.a_off, x.a_off + x.rank * x.cols, e});
        adapter.push_back({x.b_off, x.b_off + x.rows * x.rank, e});
        const int64_t n_rt = (x.rows + WN_LORA_TILE - 1) / WN_LORA_TILE, n_ct = (x.cols + WN_LORA_TILE - 1) / WN_LORA_TILE;
        if (n_rt * n_ct > 0xffffffffLL) return lora_fail(err, err_len, "wn_lora_table: entry %lld has too many tiles", e);
        tiles += n_rt * n_ct;
        reduce += (x.rank * (x.rows + x.cols) + WN_LORA_TPB - 1) / WN_LORA_TPB;
        scratch += x.rank * (n_rt * x.cols + n_ct * x.rows);
    }
    if (tiles > 0x7fffffff || reduce > 0x7fffffff) return lora_fail(err, err_len, "wn_lora_table: more than 2^31 - 1 blocks");
    for (std::vector<Range>* v : {&model, &adapter}) {
        std::sort(v->begin(), v->end(), [](const Range& a, const Range& b) { return a.lo < b.lo; });
        for (size_t i = 1; i < v->size(); ++i)
            if ((*v)[i].lo < (*v)[i - 1].hi)
                return lora_fail(err, err_len,
                                 v == &model ? "wn_lora_table: ranges of entries %lld and %lld overlap in the model buffer"
                                             : "wn_lora_table: ranges of entries %lld and %lld overlap in the adapter buffer",
                                 (*v)[i - 1].entry, (*v)[i].entry);
    }
    const int64_t words = WN_LORA_HEADER + (int64_t)WN_LORA_ENTRY_WORDS * n_entries + tiles + reduce;
    if (!table) return words;
    if (table_words < words)
        return lora_fail(err, err_len, "wn_lora_table: the table holds %lld words, %lld are needed", table_words, words);
    table[0] = WN_LORA_MAGIC, table[1] = n_entries, table[2] = tiles, table[3] = reduce, table[4] = scratch;
    table[5] = model.back().hi, table[6] = 0, table[7] = words;
    for (const Range& r : adapter) table[6] = r.hi > table[6] ? r.hi : table[6];
    for (const Range& r : model) table[5] = r.hi > table[5] ? r.hi : table[5];
    int64_t* ent = table + WN_LORA_HEADER;
    int64_t* tl = ent + (int64_t)WN_LORA_ENTRY_WORDS * n_entries;
    int64_t* rd = tl + tiles;
    int64_t soff = 0;
    for (int e = 0; e < n_entries; ++e, ent += WN_LORA_ENTRY_WORDS) {
        const WnLoraEntry& x = entries[e];
        const float s = (float)x.scale;
        unsigned bits;
        memcpy(&bits, &s, 4);
        ent[0] = x.w_off, ent[1] = x.rows, ent[2] = x.cols, ent[3] = x.rank, ent[4] = x.a_off, ent[5] = x.b_off, ent[6] = bits;
        ent[7] = soff;
        const int64_t n_rt = (x.rows + WN_LORA_TILE - 1) / WN_LORA_TILE, n_ct = (x.cols + WN_LORA_TILE - 1) / WN_LORA_TILE;
        for (int64_t i = 0; i < n_rt * n_ct; ++i) *tl++ = ((int64_t)e << 32) | i;
        for (int64_t i = 0; i < (x.rank * (x.rows + x.cols) + WN_LORA_TPB - 1) / WN_LORA_TPB; ++i) *rd++ = ((int64_t)e << 32) | i;
        soff += x.rank * (n_rt * x.cols + n_ct * x.rows);
    }
    return words;
}

const char* wn_lora_table_error(const int64_t* table, int64_t n_model, int64_t n_adapter) {
    if (!table) return "table is NULL";
    if (reinterpret_cast<uintptr_t>(table) & 7) return "table needs 8-byte alignment";
    if (table[0] != WN_LORA_MAGIC || table[1] <= 0 || table[2] <= 0 || table[3] <= 0) return "table is not what wn_lora_table wrote";
    if (table[5] > n_model) return "the table does not fit the model buffer length passed";
    if (table[6] > n_adapter) return "the table does not fit the adapter buffer length passed";
    return nullptr;
}

int wn_lora_merge_launch(const float* base, float* params, const float* adapter, const int64_t* table, const long* dev_table,
                         wn_stream_t st) {
    double elems = 0.0;
    for (int64_t e = 0; e < table[1]; ++e) elems += (double)table[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * e + 1] * (double)table[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * e + 2];
    WN_PROF("lora_merge", 0.0, 8.0 * elems, st);
    WN_LAUNCH(k_lora_merge, dim3((unsigned)table[2]), dim3(WN_LORA_TPB), 0, st, base, params, adapter, dev_table);
    return 0;
}

int wn_lora_project_launch(const float* grads, const float* adapter, float* adapter_grads, const int64_t* table,
                           const long* dev_table, float* scratch, wn_stream_t st) {
    {
        double elems = 0.0;
        for (int64_t e = 0; e < table[1]; ++e) elems += (double)table[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * e + 1] * (double)table[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * e + 2];
        WN_PROF("lora_partials", 0.0, 4.0 * elems + 4.0 * (double)table[4], st);
        int64_t rank = 1;
        for (int64_t e = 0; e < table[1]; ++e) rank = std::max(rank, table[WN_LORA_HEADER + WN_LORA_ENTRY_WORDS * e + 3]);
        const dim3 grid((unsigned)table[2]), block(WN_LORA_TPB);
        if (rank <= 4) {
            WN_LAUNCH(k_lora_partials<1>, grid, block, 0, st, grads, adapter, dev_table, scratch);
        } else if (rank <= 8) {
            WN_LAUNCH(k_lora_partials<2>, grid, block, 0, st, grads, adapter, dev_table, scratch);
        } else if (rank <= 16) {
            WN_LAUNCH(k_lora_partials<4>, grid, block, 0, st, grads, adapter, dev_table, scratch);
        } else if (rank <= 32) {
            WN_LAUNCH(k_lora_partials<8>, grid, block, 0, st, grads, adapter, dev_table, scratch);
        } else {
            WN_LAUNCH(k_lora_partials<16>, grid, block, 0, st, grads, adapter, dev_table, scratch);
        }
    }
    WN_PROF("lora_reduce", 0.0, 4.0 * (double)table[4], st);
    WN_LAUNCH(k_lora_reduce, dim3((unsigned)table[3]), dim3(WN_LORA_TPB), 0, st, scratch, dev_table, adapter_grads);
    return 0;
}
