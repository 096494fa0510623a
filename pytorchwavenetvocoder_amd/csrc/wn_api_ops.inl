// wn_api_ops.inl: op-level entry points (stand-alone layer modules, parity tests) -- part of the ONE translation unit wn_api.hip (included at its end: the entry points share its file-local
// helpers -- error text, parameter layout, workspace carving, launch contexts).  Not compiled on its own.
// ------------------------------------------------------------------------------------------
// op-level entry points
// ------------------------------------------------------------------------------------------
extern "C" int wn_op_front(const float* weight, const float* bias, const int64_t* x, float* out, float* scratch, int B, int T,
                           int Q, int R, int K, void* stream) {
    api_enter();
    WnCopy4 cp;
    cp.n0 = K; cp.n1 = Q; cp.n2 = R; cp.nl = 1;
    cp.d0 = (long)Q * R; cp.d1 = R; cp.d2 = 1; cp.dl = 0;
    cp.s0 = 1; cp.s1 = K; cp.s2 = (long)Q * K; cp.sl = 0;
    WN_TRY(wn_copy4(scratch, weight, &cp, (wn_stream_t)stream));
    WN_TRY(wn_front_gather(x, scratch, bias, out, B, T, Q, R, K, (wn_stream_t)stream));
    return rt_check("wn_op_front");
}

extern "C" int wn_op_causal_conv(const float* weight, const float* bias, const float* x, float* y, float* scratch, int B, int T,
                                 int Cin, int Cout, int K, int dilation, void* stream) {
    api_enter();
    WnCopy4 cp;  // scratch[(tap*Cin + i)*Cout + o] = W[o][i][tap]
    cp.n0 = K; cp.n1 = Cin; cp.n2 = Cout; cp.nl = 1;
    cp.s0 = 1; cp.s1 = K; cp.s2 = (long)Cin * K; cp.sl = 0;
    cp.d0 = (long)Cin * Cout; cp.d1 = Cout; cp.d2 = 1; cp.dl = 0;
    WN_TRY(wn_copy4(scratch, weight, &cp, (wn_stream_t)stream));
    WnGemmArgs g = wn_gemm_default();
    g.M = Cout; g.N = T; g.K = K * Cin;
    g.A = scratch; g.lda = Cout;
    g.B = x; g.ldb = T; g.b_zstride = (long)Cin * T; g.b_clen = T;
    g.b_seg_len = Cin; g.b_seg_stride = 0; g.b_shift0 = (K - 1) * dilation; g.b_shift_step = -dilation;
    g.C = y; g.ldc = T; g.c_zstride = (long)Cout * T;
    g.bias = bias; g.nbatch = B;
    WN_TRY(wn_gemm_launch(&g, (wn_stream_t)stream));
    return rt_check("wn_op_causal_conv");
}

// Backward of CausalConv1d (autograd of wavenet.py:95-121) as three contractions of the same exact-f32 kernel family:
//   dx[b,i,t]  = sum_k sum_o W[o,i,k] dy[b,o,t + (K-1-k)d]            (taps transposed: dy read AHEAD, zero beyond T)
//   dW[o,i,k]  = sum_b sum_t dy[b,o,t] x[b,i,t - (K-1-k)d]            (k = time; per-(b, k-chunk) partials, fixed-order sum)
//   db[o]      = sum_b sum_t dy[b,o,t]                                 (row sums of the same launch)
// Any of dx / dw / db may be NULL.  scratch: wn_op_causal_conv_backward_scratch_floats() floats.
static void ccb_plan(int B, int T, int* ksplit, int* kchunk) {
    int ks = (T + 4095) / 4096;
    if (ks * B > 512) ks = 512 / B;
    if (ks < 1) ks = 1;
    int kc = ((T + ks - 1) / ks + 31) / 32 * 32;
    if (kc < 32) kc = 32;
    *kchunk = kc;
    *ksplit = (T + kc - 1) / kc;
}

extern "C" long wn_op_causal_conv_backward_scratch_floats(int B, int T, int Cin, int Cout, int K) {
    if (B < 1 || T < 1 || Cin < 1 || Cout < 1 || K < 1) return 0;
    int ks, kc;
    ccb_plan(B, T, &ks, &kc);
    const long nz = (long)B * ks;
    return (long)K * Cin * Cout + nz * Cout * K * Cin + nz * Cout + 64;
}

extern "C" int wn_op_causal_conv_backward(const float* weight, const float* x, const float* dy, float* dx, float* dw, float* db,
                                          float* scratch, int B, int T, int Cin, int Cout, int K, int dilation, void* stream) {
    api_enter();
    if (!weight || !x || !dy || !scratch || B < 1 || T < 1 || Cin < 1 || Cout < 1 || K < 1 || dilation < 1) return fail(1, "bad argument");
    wn_stream_t st = (wn_stream_t)stream;
    if (dx) {
        WnCopy4 cp;  // scratch[(tap*Cout + o)*Cin + i] = W[o][i][tap]
        cp.n0 = K; cp.n1 = Cout; cp.n2 = Cin; cp.nl = 1;
        cp.s0 = 1; cp.s1 = (long)Cin * K; cp.s2 = K; cp.sl = 0;
        cp.d0 = (long)Cout * Cin; cp.d1 = Cin; cp.d2 = 1; cp.dl = 0;
        WN_TRY(wn_copy4(scratch, weight, &cp, st));
        WnGemmArgs g = wn_gemm_default();
        g.M = Cin; g.N = T; g.K = K * Cout;
        g.A = scratch; g.lda = Cin;
        g.B = dy; g.ldb = T; g.b_zstride = (long)Cout * T; g.b_clen = T;
        g.b_seg_len = Cout; g.b_seg_stride = 0; g.b_shift0 = -(K - 1) * dilation; g.b_shift_step = dilation;
        g.C = dx; g.ldc = T; g.c_zstride = (long)Cin * T;
        g.nbatch = B; g.tag = "op_causal_conv_dx";
        WN_TRY(wn_gemm_launch(&g, st));
    }
    if (dw || db) {
        int ks, kc;
        ccb_plan(B, T, &ks, &kc);
        const int nz = B * ks;
        const int N = K * Cin;
        float* partial = scratch + (long)K * Cin * Cout;
        float* rs_partial = partial + (long)nz * Cout * N;
        WnGemmArgs g = wn_gemm_default();
        g.M = Cout; g.N = N; g.K = T;
        g.A = dy; g.lda = T; g.a_zstride = (long)Cout * T; g.a_kmajor = 1;
        g.B = x; g.ldb = T; g.b_zstride = (long)Cin * T; g.b_kmajor = 1; g.b_clen = T;
        g.b_seg_len = Cin; g.b_seg_stride = 0; g.b_shift0 = (K - 1) * dilation; g.b_shift_step = -dilation;
        g.C = partial; g.ldc = N; g.c_zstride = (long)Cout * N;
        g.nbatch = B; g.ksplit = ks; g.kchunk = kc;
        g.a_rowsum = db ? rs_partial : nullptr;
        g.tag = "op_causal_conv_dw";
        WN_TRY(wn_gemm_launch(&g, st));
        if (dw) {   // dW[o][i][tap] = sum_z partial[z][o][tap*Cin + i]
            WnReduceArgs r = reduce_plain(partial, nz, Cout, N, dw, (long)Cin * K, K);
            r.n_seg = Cin; r.n_seg_stride = 1;
            WN_TRY(wn_reduce(&r, st));
        }
        if (db) {
            const WnReduceArgs q = reduce_plain(rs_partial, nz, Cout, 1, db, 1, 0);
            WN_TRY(wn_reduce(&q, st));
        }
    }
    return rt_check("wn_op_causal_conv_backward");
}

// UpSampling.forward (wavenet.py:141-154): y[b][c][f U + j] = x[b][c][f] w[j] + bias  (ConvTranspose2d (1,U)/(1,U), one kernel
// shared by all channels); weight [U], bias [1] or NULL.
extern "C" int wn_op_upsampling(const float* weight, const float* bias, const float* x, float* y, int B, int C, int F, int U,
                                void* stream) {
    api_enter();
    if (!weight || !x || !y || B < 1 || C < 1 || F < 1 || U < 1) return fail(1, "bad argument");
    WN_TRY(wn_decode_ctx_aux_rows(x, weight, bias, y, B, C, F, U, F * U, 0, 0, (wn_stream_t)stream));
    return rt_check("wn_op_upsampling");
}

// dst (B, C, R) = src (B, R, C) transposed: the layout change between the reference's logits (B, T, Q) (wavenet.py:522) and the
// kernels' (B, Q, T), for a gradient that arrives from an external loss (nets/wavenet.py: the autograd bridge).
extern "C" int wn_op_transpose_last2(const float* src, float* dst, int B, int R, int C, void* stream) {
    api_enter();
    if (!src || !dst || src == dst || B < 1 || R < 1 || C < 1 || (long)((R + 31) / 32) > 65535 || B > 65535) return fail(1, "bad argument");
    WN_TRY(wn_transpose_last2(src, dst, B, R, C, (wn_stream_t)stream));
    return rt_check("wn_op_transpose_last2");
}

extern "C" int wn_op_gemm(const struct WnGemmArgs* args, void* stream) {
    api_enter();
    WN_TRY(wn_gemm_launch(args, (wn_stream_t)stream));
    return rt_check("wn_op_gemm");
}

// The per-sequence reduction of the scoring entry points on its own: row_out[b] = sum of partial[b * nblk .. (b + 1) * nblk),
// acc[0] (nullable, double) += the sum of the row sums as they are in double, before their rounding to float.
extern "C" int wn_op_row_sums(const float* partial, int B, int nblk, float* row_out, double* acc, void* stream) {
    api_enter();
    if (!partial || !row_out || B < 1 || nblk < 1) return fail(1, "bad argument");
    WN_TRY(wn_row_sums(partial, B, nblk, row_out, acc, 0, (wn_stream_t)stream));
    return rt_check("wn_op_row_sums");
}

// a[i] <-> b[i] in place (FusedAdam.ema_weights: the weights and their moving average change places, one launch each way).
extern "C" int wn_op_swap(float* a, float* b, int64_t n, void* stream) {
    api_enter();
    if (!a || !b || n <= 0) return fail(1, "bad wn_op_swap argument");
    if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(b) & 3)) return fail(1, "wn_op_swap: the buffers need 4-byte alignment");
    if (ranges_overlap(a, b, n)) return fail(1, "wn_op_swap: the two ranges overlap");
    WN_TRY(wn_swap(a, b, (long)n, (wn_stream_t)stream));
    return rt_check("wn_op_swap");
}

// Gradient accumulation over micro-batches: WN_ACCUM_SET acc = grad, WN_ACCUM_ADD acc = acc + grad, WN_ACCUM_FINISH
// grad = acc + grad (WaveNet.loss_and_backward(micro_step=(i, A)); a pointer and a length, so a gradient bucket is a call).
extern "C" int wn_op_accumulate(float* acc, float* grad, int64_t n, int mode, void* stream) {
    api_enter();
    if (!acc || !grad || n <= 0) return fail(1, "bad wn_op_accumulate argument");
    if (mode != WN_ACCUM_SET && mode != WN_ACCUM_ADD && mode != WN_ACCUM_FINISH)
        return fail(1, "wn_op_accumulate: mode %d is none of WN_ACCUM_SET, WN_ACCUM_ADD, WN_ACCUM_FINISH", mode);
    if ((reinterpret_cast<uintptr_t>(acc) & 3) || (reinterpret_cast<uintptr_t>(grad) & 3)) return fail(1, "wn_op_accumulate: the buffers need 4-byte alignment");
    if (ranges_overlap(acc, grad, n)) return fail(1, "wn_op_accumulate: the two ranges overlap");
    WN_TRY(wn_grad_accumulate(acc, grad, (long)n, mode, (wn_stream_t)stream));
    return rt_check("wn_op_accumulate");
}

// ------------------------------------------------------------------------------------------
// Low-rank adapters (ABI v22): the host table and the two fused operations of wn_lora.hip.
extern "C" int64_t wn_lora_table(const WnLoraEntry* entries, int n_entries, int64_t n_model, int64_t n_adapter, int64_t* table,
                                 int64_t table_words) {
    g_err[0] = 0;   // pure host code: no runtime call to clear
    if (table && (reinterpret_cast<uintptr_t>(table) & 7)) return fail(1, "wn_lora_table: table needs 8-byte alignment"), -1;
    return wn_lora_build_table(entries, n_entries, n_model, n_adapter, table, table_words, g_err, sizeof(g_err));
}

extern "C" int64_t wn_lora_scratch_floats(const int64_t* table) {
    g_err[0] = 0;
    if (const char* why = wn_lora_table_error(table, INT64_MAX, INT64_MAX)) return fail(1, "wn_lora_scratch_floats: %s", why), -1;
    return table[4];
}

extern "C" int wn_lora_merge(const float* base, float* params, int64_t n_model, const float* adapter, int64_t n_adapter,
                             const int64_t* table, const int64_t* dev_table, void* stream) {
    api_enter();
    if (!base || !params || !adapter || !dev_table || n_model <= 0 || n_adapter <= 0) return fail(1, "bad wn_lora_merge argument (NULL pointer or a length <= 0)");
    if ((reinterpret_cast<uintptr_t>(base) & 3) || (reinterpret_cast<uintptr_t>(params) & 3) || (reinterpret_cast<uintptr_t>(adapter) & 3) ||
        (reinterpret_cast<uintptr_t>(dev_table) & 7))
        return fail(1, "wn_lora_merge: the buffers need 4-byte, the tables 8-byte alignment");
    if (const char* why = wn_lora_table_error(table, n_model, n_adapter)) return fail(1, "wn_lora_merge: %s", why);
    if (ranges_overlap(base, params, n_model)) return fail(1, "wn_lora_merge: base overlaps params");
    WN_TRY(wn_lora_merge_launch(base, params, adapter, table, reinterpret_cast<const long*>(dev_table), (wn_stream_t)stream));
    return rt_check("wn_lora_merge");
}

extern "C" int wn_lora_project(const float* grads, int64_t n_model, const float* adapter, float* adapter_grads, int64_t n_adapter,
                               const int64_t* table, const int64_t* dev_table, float* scratch, int64_t scratch_floats, void* stream) {
    api_enter();
    if (!grads || !adapter || !adapter_grads || !dev_table || !scratch || n_model <= 0 || n_adapter <= 0)
        return fail(1, "bad wn_lora_project argument (NULL pointer or a length <= 0)");
    if ((reinterpret_cast<uintptr_t>(grads) & 3) || (reinterpret_cast<uintptr_t>(adapter) & 3) || (reinterpret_cast<uintptr_t>(adapter_grads) & 3) ||
        (reinterpret_cast<uintptr_t>(scratch) & 3) || (reinterpret_cast<uintptr_t>(dev_table) & 7))
        return fail(1, "wn_lora_project: the buffers need 4-byte, the tables 8-byte alignment");
    if (const char* why = wn_lora_table_error(table, n_model, n_adapter)) return fail(1, "wn_lora_project: %s", why);
    if (scratch_floats < table[4]) return fail(1, "wn_lora_project: scratch holds %lld floats, wn_lora_scratch_floats asks for %lld", (long long)scratch_floats, (long long)table[4]);
    if (ranges_overlap(adapter, adapter_grads, n_adapter)) return fail(1, "wn_lora_project: adapter overlaps adapter_grads");
    WN_TRY(wn_lora_project_launch(grads, adapter, adapter_grads, table, reinterpret_cast<const long*>(dev_table), scratch,
                                  (wn_stream_t)stream));
    return rt_check("wn_lora_project");
}
