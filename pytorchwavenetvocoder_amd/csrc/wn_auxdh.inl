// wn_auxdh.inl: the gradient with respect to the aux features, dh = sum_l Waux_l^T dG_l -- part of wn_elem.hip (included at its
// end).  Not compiled on its own.
//
//   dh[b][m][n] = sum_k W[m][k] * S[k / R2][b][k % R2][n]      k = l * R2 + c,  K = L * R2
//
// W = the packed aux weights of the forward pass (waux_f: [a][l * 2R + c]), S = dG (upsampling layer: frame rate, n < F) or dP
// (no upsampling layer: n < T) of every layer.  f32-input MFMA (v_mfma_f32_16x16x4_f32): exact fp32 products, fp32 accumulation.
//
// One wave owns 64 consecutive columns and all rows of an m-group (MB blocks of 16 rows) of one batch item, and walks its k
// range in steps of 16.  Lane (g = l >> 4, j = l & 15) of step k0 loads W[m][k0 + 4g .. + 3] of every row block (one 16-byte
// load per row block) and S rows k0 + 4g + s (s = 0..3) at columns n0 + 4j .. + 3 (four rows x 256 contiguous bytes per load
// instruction).  MFMA s of the step then contracts k = k0 + 4g + s for g = 0..3, and accumulator q (of 4) holds the columns
// n0 + 4j + q: the k order inside a step and the column order inside a tile are permutations that the two operands share.
// Every output element is one lane's fixed chain of MFMAs over its k range -- no atomics, the same bits on every run.
// Split-K (grid.z): the partial of chunk z goes to part[z]; k_aux_dh_sum adds the chunks in the order z = 0, 1, ...
#define WN_DH_TPB 256

static __device__ __forceinline__ void dh_ld4(const float* p, float (&v)[4]) {
    const wn_f4 q = wn_ld4_unaligned(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

// row k of the B operand, columns [n, n + 4) (zeros beyond ncol)
static __device__ __forceinline__ void dh_ld_row(const float* S, long s_lstride, int R2, int k, int kend, long n, int N, bool vec,
                                                 float (&v)[4]) {
    if (k >= kend || n >= N) {
        v[0] = v[1] = v[2] = v[3] = 0.0f;
        return;
    }
    const int l = k / R2;
    const float* p = S + (long)l * s_lstride + (long)(k - l * R2) * N + n;
    if (vec) {
        dh_ld4(p, v);
    } else {
        WN_UNROLL
        for (int q = 0; q < 4; ++q) v[q] = (n + q < N) ? p[q] : 0.0f;
    }
}

// W[m][k0 .. k0 + 3] (zeros beyond M / kend)
static __device__ __forceinline__ void dh_ld_w(const float* W, int M, int K, int m, int k, int kend, float (&v)[4]) {
    if (m >= M || k >= kend) {
        v[0] = v[1] = v[2] = v[3] = 0.0f;
        return;
    }
    const float* p = W + (long)m * K + k;
    if (k + 4 <= kend) {
        dh_ld4(p, v);
    } else {
        WN_UNROLL
        for (int q = 0; q < 4; ++q) v[q] = (k + q < kend) ? p[q] : 0.0f;
    }
}

// grid: x = column tiles of 64 / 4 waves, y = batch item, z = k chunk * m-groups + m-group
template <int MB>
__global__ __launch_bounds__(WN_DH_TPB) void k_aux_dh(const float* __restrict__ W, int M, int K, const float* __restrict__ S,
                                                      long s_lstride, long s_bstride, int R2, int N, int kchunk, int mgroups,
                                                      float* __restrict__ out, long out_zstride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, j = lane & 15;
    const long n0 = ((long)blockIdx.x * (WN_DH_TPB / 64) + wave) * 64;
    if (n0 >= N) return;   // (wave-uniform: a whole wave leaves)
    const int b = blockIdx.y;
    const int mg = blockIdx.z % mgroups, kz = blockIdx.z / mgroups;
    const int m0 = mg * MB * 16;
    const int kbeg = kz * kchunk;
    const int kend = kbeg + kchunk < K ? kbeg + kchunk : K;
    S += (long)b * s_bstride;
    const long n = n0 + 4 * j;
    const bool vec = (N & 3) == 0;   // 16-byte row segments (N % 4 == 0: all four columns valid together)
    f32x4 acc[MB][4];
    WN_UNROLL
    for (int mb = 0; mb < MB; ++mb)
        WN_UNROLL
        for (int q = 0; q < 4; ++q)
            WN_UNROLL
            for (int r = 0; r < 4; ++r) acc[mb][q][r] = 0.0f;
    float a[MB][4], s4[4][4];
    // software pipeline: the operands of step k0 + 16 are loaded while step k0 runs on the matrix cores
    WN_UNROLL
    for (int mb = 0; mb < MB; ++mb) dh_ld_w(W, M, K, m0 + 16 * mb + j, kbeg + 4 * g, kend, a[mb]);
    WN_UNROLL
    for (int s = 0; s < 4; ++s) dh_ld_row(S, s_lstride, R2, kbeg + 4 * g + s, kend, n, N, vec, s4[s]);
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        float an[MB][4], sn[4][4];
        const int k1 = k0 + 16;
        WN_UNROLL
        for (int mb = 0; mb < MB; ++mb) dh_ld_w(W, M, K, m0 + 16 * mb + j, k1 + 4 * g, kend, an[mb]);
        WN_UNROLL
        for (int s = 0; s < 4; ++s) dh_ld_row(S, s_lstride, R2, k1 + 4 * g + s, kend, n, N, vec, sn[s]);
        WN_UNROLL
        for (int s = 0; s < 4; ++s)
            WN_UNROLL
            for (int mb = 0; mb < MB; ++mb)
                WN_UNROLL
                for (int q = 0; q < 4; ++q) acc[mb][q] = mfma16(a[mb][s], s4[s][q], acc[mb][q]);
        WN_UNROLL
        for (int mb = 0; mb < MB; ++mb)
            WN_UNROLL
            for (int e = 0; e < 4; ++e) a[mb][e] = an[mb][e];
        WN_UNROLL
        for (int s = 0; s < 4; ++s)
            WN_UNROLL
            for (int e = 0; e < 4; ++e) s4[s][e] = sn[s][e];
    }
    // accumulator register r of lane (g, j): row 4 g + r of the block, column j of the 16 -> memory column n0 + 4 j + q
    float* o = out + (long)kz * out_zstride + (long)b * M * N;
    WN_UNROLL
    for (int mb = 0; mb < MB; ++mb)
        WN_UNROLL
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * mb + 4 * g + r;
            if (m >= M) continue;
            float* row = o + (long)m * N;
            WN_UNROLL
            for (int q = 0; q < 4; ++q)
                if (n + q < N) row[n + q] = acc[mb][q][r];
        }
}

// out[i] = sum_{z < nz} part[z * zstride + i], z ascending
__global__ __launch_bounds__(WN_DH_TPB) void k_aux_dh_sum(const float* __restrict__ part, int nz, long zstride, long n,
                                                          float* __restrict__ out) {
    const long i = (long)blockIdx.x * WN_DH_TPB + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int z = 1; z < nz; ++z) s += part[(long)z * zstride + i];
    out[i] = s;
}

// k chunk of a launch: about two waves per SIMD (256 CUs x 4), chunks of at least 64 k, the partials within the scratch
static int aux_dh_kchunk(int M, int K, int N, int B, long scratch_floats) {
    const int mb = (M + 15) / 16;
    const int mgroups = (mb + 7) / 8;
    const long waves = (long)((N + 63) / 64) * B * mgroups;
    long ks = (2048 + waves - 1) / waves;
    const long maxks = (K + 63) / 64;
    if (ks > maxks) ks = maxks;
    const long per = (long)B * M * N;
    if (ks > 1 && ks * per > scratch_floats) ks = scratch_floats / per;
    if (ks < 1) ks = 1;
    const int kchunk = (int)((K + ks - 1) / ks);
    return (kchunk + 15) / 16 * 16;   // (ceil(K / kchunk) <= ks)
}

int wn_aux_dh(const float* W, int M, int K, const float* S, long s_lstride, long s_bstride, int R2, int N, int B, float* dh,
              float* scratch, long scratch_floats, wn_stream_t st) {
    if (M < 1 || K < 1 || N < 1 || B < 1 || R2 < 1 || K % R2 != 0) return 1;
    const int kchunk = aux_dh_kchunk(M, K, N, B, scratch_floats);
    const int nz = (K + kchunk - 1) / kchunk;
    const int mbt = (M + 15) / 16;
    const int MB = mbt < 8 ? mbt : 8;
    const int mgroups = (mbt + 7) / 8;
    const long per = (long)B * M * N;
    float* out = nz > 1 ? scratch : dh;
    if (nz > 1 && (long)nz * per > scratch_floats) return 2;
    const dim3 grid((unsigned)(((N + 63) / 64 + WN_DH_TPB / 64 - 1) / (WN_DH_TPB / 64)), (unsigned)B, (unsigned)(nz * mgroups));
    {
        WN_PROF("aux_dh", 2.0 * M * K * N * B, ((double)K * N * B + (double)M * N * B * nz) * 4.0, st);
        switch (MB) {
#define WN_DH_CASE(n) \
            case n: WN_LAUNCH((k_aux_dh<n>), grid, dim3(WN_DH_TPB), 0, st, W, M, K, S, s_lstride, s_bstride, R2, N, kchunk, mgroups, out, per); break;
            WN_DH_CASE(1) WN_DH_CASE(2) WN_DH_CASE(3) WN_DH_CASE(4) WN_DH_CASE(5) WN_DH_CASE(6) WN_DH_CASE(7) WN_DH_CASE(8)
#undef WN_DH_CASE
            default: return 3;
        }
    }
    if (nz > 1) {
        WN_PROF("aux_dh_sum", 0.0, (double)per * (nz + 1) * 4.0, st);
        WN_LAUNCH(k_aux_dh_sum, dim3((unsigned)((per + WN_DH_TPB - 1) / WN_DH_TPB)), dim3(WN_DH_TPB), 0, st, scratch, nz, per, per, dh);
    }
    return 0;
}
