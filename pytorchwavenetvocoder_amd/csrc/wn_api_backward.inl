// wn_api_backward.inl: wn_backward / wn_backward_window (autograd backward, train.py:538), wn_adam_step (train.py:457-460,539) -- part of the ONE translation unit wn_api.hip (included at its end: the entry points share its file-local
// helpers -- error text, parameter layout, workspace carving, launch contexts).  Not compiled on its own.
// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
static const int NO_SEG = 0x7fffffff;   // m_seg / n_seg of an axis that is not cut into segments

struct DwOut {          // destination mapping of a weight-gradient (see WnReduceArgs)
    float* out;
    int m_seg, n_seg;
    long m_seg_stride, m_stride, n_seg_stride, n_stride;
    const float* addend_m;
    const float* addend_scale_ptr;
    float* rowsum_out;  // nullable: [M] contiguous destination of sum_k A(m,k)
    long out_lstride, addend_lstride, rowsum_lstride;  // per layer of a batched launch
};
// Row m goes to (m / m_seg) * m_seg_stride + (m % m_seg) * m_stride, column n likewise (NO_SEG: one segment); one layer, no addend
static DwOut dw_out_seg(float* out, int m_seg, long m_seg_stride, long m_stride, int n_seg, long n_seg_stride, long n_stride,
                        float* rowsum_out) {
    DwOut o;
    o.out = out; o.m_seg = m_seg; o.n_seg = n_seg;
    o.m_seg_stride = m_seg_stride; o.m_stride = m_stride; o.n_seg_stride = n_seg_stride; o.n_stride = n_stride;
    o.addend_m = nullptr; o.addend_scale_ptr = nullptr; o.rowsum_out = rowsum_out;
    o.out_lstride = 0; o.addend_lstride = 0; o.rowsum_lstride = 0;
    return o;
}
static DwOut dw_out_plain(float* out, long ld, float* rowsum_out) { return dw_out_seg(out, NO_SEG, 0, ld, NO_SEG, 0, 1, rowsum_out); }

// fixed-order sum of `nz` partial [M][N] matrices into out[m * m_stride + n * n_stride]: one layer, no segments, no second level
static WnReduceArgs reduce_plain(const float* partial, int nz, int M, int N, float* out, long m_stride, long n_stride) {
    WnReduceArgs r;
    r.partial = partial; r.nz = nz; r.M = M; r.N = N;
    r.out = out; r.m_seg = NO_SEG; r.n_seg = NO_SEG;
    r.m_seg_stride = 0; r.m_stride = m_stride; r.n_seg_stride = 0; r.n_stride = n_stride;
    r.scale = 1.0f; r.accumulate = 0; r.addend_m = nullptr; r.addend_scale_ptr = nullptr;
    r.scratch = nullptr; r.scratch_floats = 0; r.nl = 1; r.out_lstride = 0; r.addend_lstride = 0;
    return r;
}

// dW[l][m][n] = sum_{b, k} A_{l,b}(m,k) * B_{l,b}(n,k)   (k = time) for nl layers in ONE launch,
// split over (layer, b, k-chunks) and reduced in a fixed order.
// fixed-order sum of `nz` partial [M][N] matrices per layer (and of the [M] row-sum partials) into their mapped destinations
static int dw_reduce(const Ctx& c, const float* partial, const float* rs_partial, int nz, int M, int N, const DwOut& o, int nl) {
    WnReduceArgs r = reduce_plain(partial, nz, M, N, o.out, o.m_stride, o.n_stride);
    r.m_seg = o.m_seg; r.n_seg = o.n_seg; r.m_seg_stride = o.m_seg_stride; r.n_seg_stride = o.n_seg_stride;
    r.addend_m = o.addend_m; r.addend_scale_ptr = o.addend_scale_ptr;
    r.scratch = c.ws + c.w.red_scratch; r.scratch_floats = c.w.red_scratch_floats;
    r.nl = nl; r.out_lstride = o.out_lstride; r.addend_lstride = o.addend_lstride;
    WN_TRY(wn_reduce(&r, c.st));
    if (o.rowsum_out) {
        WnReduceArgs q = reduce_plain(rs_partial, nz, M, 1, o.rowsum_out, 1, 0);
        q.scratch = r.scratch; q.scratch_floats = r.scratch_floats;
        q.nl = nl; q.out_lstride = o.rowsum_lstride;
        WN_TRY(wn_reduce(&q, c.st));
    }
    return 0;
}

static int dw_gemm(const Ctx& c, WnGemmArgs g, const DwOut& o, int nl = 1) {
    const DwPlan p = dw_plan(g.M, g.N, g.K, c.B * nl);
    const int nz_layer = p.ksplit * c.B;
    g.a_kmajor = 1; g.b_kmajor = 1;
    g.nlayer = nl; g.nbatch = c.B; g.ksplit = p.ksplit; g.kchunk = p.kchunk;
    g.C = c.ws + c.w.partial; g.ldc = g.N; g.c_zstride = (long)g.M * g.N;
    g.a_rowsum = o.rowsum_out ? c.ws + c.w.rs_partial : nullptr;
    if (c.r.split_bf16 && wn_gemm6_dw_eligible(&g)) {
        if (c.dw_f16_mul != 0.0f) {
            // fp16 pair split; the six-product launch behind it returns at once unless a gradient left fp16's range
            WN_TRY(wn_gemm6_dw_launch(&g, 3, c.dw_f16_mul, c.dw_ovf, c.st));
            WN_TRY(wn_gemm6_dw_launch(&g, 6, 0.0f, c.dw_ovf, c.st));
        } else {
            WN_TRY(wn_gemm6_dw_launch(&g, c.dw_products, 0.0f, nullptr, c.st));
        }
    } else
        WN_TRY(wn_gemm_launch(&g, c.st));
    return dw_reduce(c, c.ws + c.w.partial, c.ws + c.w.rs_partial, nz_layer, g.M, g.N, o, nl);
}

// skip_1x1.l.bias = rowsum(dSkip), which the reduction left in tmpS, for every layer of the stack
static int skip_bias_all(const Ctx& c, float* grads) {
    const Dims& d = c.d;
    WnCopy4 cp;
    cp.n0 = 1; cp.n1 = 1; cp.n2 = d.S; cp.nl = d.L;
    cp.s0 = 0; cp.s1 = 0; cp.s2 = 1; cp.sl = 0;
    cp.d0 = 0; cp.d1 = 0; cp.d2 = 1; cp.dl = c.y.ls_skip;
    return wn_copy4(grads + c.p_skip(0) + (long)d.S * d.R, c.ws + c.w.tmpS, &cp, c.st);
}

extern "C" int wn_backward(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                           const float* dlogits, float* grads, void* wsp, size_t ws_bytes, void* const* events, int n_events,
                           int lpb, int flags, void* stream) {
    return wn_backward_window(cfg, B, T, params, x, h, dlogits, 0, grads, wsp, ws_bytes, events, n_events, lpb, flags, stream);
}

// grads == NULL (wn_backward_dh only): the data gradients and dh alone -- no weight-gradient launch, no reduction of one, and no
// scale of the fp16 pair weight gradients (the data contractions of WN_FLAG_MM_F16PAIR still take theirs).  dh != NULL: dL/dh
// (wn_auxdh.inl) after the last flush group, on its stream; the flush groups then keep dG of every layer (at its own offset).
//
// Frozen parameters (wn_backward_needs, ABI v16): `first_layer` is the lowest layer whose own tensors hold a
// trainable one (L: none) and `needs` says which of the post-net, the front conv and the upsampling layer train.  The pass then
// stops where nothing below needs it: the chain runs from L - 1 down to first_layer and the launch that would produce
// dX_{first_layer} is left out (unless first_layer == 0 and the front conv trains); flush groups and buckets are counted from the
// top as always, so a group wholly at or above first_layer is the full pass's group, launch for launch, and the lowest one is cut
// at first_layer; a bucket whose layers were all left out still gets its event where the walk reaches it.  Nothing is left out
// inside a computed layer.  The other three entry points pass first_layer = 0 and WN_NEED_ALL: the launches of before.
static int backward_impl(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                         const float* dlogits, int t_first, float* grads, float* dh, void* wsp, size_t ws_bytes,
                         void* const* events, int n_events, int lpb, int flags, void* stream, int first_layer = 0,
                         int needs = WN_NEED_ALL) {
    Ctx c;
    WN_TRY(make_ctx(&c, cfg, B, T, wsp, ws_bytes, flags, stream));
    if (!params || !x || !h || !dlogits || (!grads && !dh)) return fail(1, "NULL argument");
    c.params = params;
    if (t_first < 0 || t_first >= T) return fail(1, "t_first=%d outside [0,%d)", t_first, T);
    const bool wgrad = grads != nullptr;
    const int fl = first_layer;
    if (fl < 0 || fl > c.d.L) return fail(1, "first_layer=%d outside [0,%d]", fl, c.d.L);
    if (needs & ~WN_NEED_ALL) return fail(1, "needs=%d holds unknown bits", needs);
    if (fl > 0 && (dh || !wgrad)) return fail(1, "first_layer=%d with dh: dL/dh needs every layer (first_layer = 0)", fl);
    if (fl > 0 && (needs & (WN_NEED_FRONT | WN_NEED_UP)))
        return fail(1, "first_layer=%d with the front conv or the upsampling layer trainable: both need every layer (first_layer = 0)", fl);
    const bool need_post = wgrad && (needs & WN_NEED_POST), need_front = (needs & WN_NEED_FRONT) != 0,
               need_up = (needs & WN_NEED_UP) != 0;
    const bool any_below_logits = fl < c.d.L || need_post;   // false: nothing at all reads dO2 / dSkip
    if (c.dw_f16_mode && (wgrad || c.r.mm_f16)) {   // before the side stream forks: overflow word := 0, a_mul := the scale of this call's gradient (wn_elem.h)
        const int tw0 = (t_first / 128) * 128;
        float* words = c.ws + c.w.dw_ovf;
        if (c.dw_f16_mode == 1) {
            WN_TRY(wn_dw_prepare(words, ldexpf(1.0f, ((flags >> WN_FLAG_DW_F16_EXP_SHIFT) & 63) + WN_DW_F16_HEADROOM), nullptr, 0, WN_DW_F16_HEADROOM, c.st));
        } else if (c.dw_f16_mode == 2) {
            WN_TRY(wn_dw_prepare(words, 0.0f, nullptr, 0, WN_DW_F16_HEADROOM, c.st));
        } else {   // nobody vouches for the size of this gradient: one pass over it (the loss window's columns)
            const long rows = (long)B * c.d.Qo;
            const int nchunk = (T - tw0 + 4095) / 4096;
            if (rows * nchunk > c.w.amax_partial_floats) return fail(1, "dlogits scan: partial buffer too small");
            WN_TRY(wn_absmax_rows(dlogits, rows, T, tw0, T - tw0, c.ws + c.w.amax_partial, c.st));
            WN_TRY(wn_dw_prepare(words, 0.0f, c.ws + c.w.amax_partial, (int)(rows * nchunk), WN_DW_F16_HEADROOM, c.st));
        }
    }
    // WN_FLAG_REPACK: `params` changed since the forward call (or the caller cannot tell): rebuild every re-laid-out /
    // pre-split weight set of the workspace from the buffer given HERE, so that the backward contractions use one
    // consistent set of weights (the saved activations are the forward pass's own either way).
    if (flags & WN_FLAG_REPACK) WN_TRY(pack_weights(c, params));
    // Loss window.  The loss of train.py:534-536 covers [:, receptive_field:], so dlogits is exactly zero in front of it, and
    // everything between the logits and the residual stack is pointwise in time: dO2, dSkip and the skip part of every
    // layer's dZ are zero there too, and those columns contribute nothing to the post-net / skip weight gradients.  The
    // contractions of this part run over [t0, T) only (t0 = t_first rounded down to a whole 128-column tile, so that every
    // row keeps its alignment); dSkip is zero-filled in front of t0 and the chain kernel takes dZs as zero there: the chain
    // itself needs every position (dX_l[t] depends on dP_l[t + dilation]).  13 % less matrix work in these launches at the benchmark's geometry.
    const int t0 = (t_first / 128) * 128;
    const int Tw = T - t0;
    // c = the data chain on the caller's stream; cs = the weight gradients, on the side stream unless serial
    SideLock side((flags & WN_FLAG_BWD_OVERLAP) && !wn_prof_is_on(), c.st);
    Ctx cs = c;
    if (side.rt) cs.st = side.rt->st;
    const Dims& d = c.d;
    const Lay& y = c.y;
    const Ws& w = c.w;
    float* ws = c.ws;
    const int F = w.F, Ue = d.U > 0 ? d.U : 1;
    if (lpb < 1) lpb = d.L;
    const int nb = wn_num_buckets(cfg, lpb);
    if (events && n_events < nb) return fail(1, "need %d bucket events, got %d", nb, n_events);
    int bucket = 0;

    // ---- post-net backward (wavenet.py:518-523 reversed) ----
    if (any_below_logits) {   // dO2 = W2^T dlogits, masked by relu'(O2)
        WnGemmArgs g = wn_gemm_default();
        g.M = d.S; g.N = Tw; g.K = d.Qo;
        g.A = params + y.post2_w; g.lda = d.S;
        g.B = dlogits + t0; g.ldb = T; g.b_zstride = (long)d.Qo * T; g.b_clen = Tw;
        g.C = ws + w.dO2 + t0; g.ldc = T; g.c_zstride = (long)d.S * T;
        g.E = ws + w.O2 + t0; g.lde = T; g.e_zstride = (long)d.S * T;
        g.nbatch = B; g.tag = "bwd_post2_dx";
        WN_TRY(fw_gemm(c, g, nullptr, nullptr, t0, true));
    }
    if (any_below_logits) {   // dSkip = W1^T dO2, masked by relu'(skip-sum)
        WnGemmArgs g = wn_gemm_default();
        g.M = d.S; g.N = Tw; g.K = d.S;
        g.A = params + y.post1_w; g.lda = d.S;
        g.B = ws + w.dO2 + t0; g.ldb = T; g.b_zstride = (long)d.S * T; g.b_clen = Tw;
        g.C = ws + w.dSk + t0; g.ldc = T; g.c_zstride = (long)d.S * T;
        g.E = ws + w.O1 + t0; g.lde = T; g.e_zstride = (long)d.S * T;
        g.nbatch = B; g.tag = "bwd_post1_dx";
        WN_TRY(fw_gemm(c, g, nullptr, nullptr, t0, true));
        if (t0 > 0) WN_TRY(wn_fill_cols(ws + w.dSk, (long)B * d.S, T, t0, c.st));
    }
    WN_TRY(side_link(side.rt, c.st, cs.st));  // fork: dO2, dSkip (and everything before this call) are ready
    if (need_post) {   // d conv_post_2.{weight,bias}
        WnGemmArgs g = wn_gemm_default();
        g.M = d.Qo; g.N = d.S; g.K = Tw;
        g.A = dlogits + t0; g.lda = T; g.a_zstride = (long)d.Qo * T;
        g.B = ws + w.O2 + t0; g.ldb = T; g.b_zstride = (long)d.S * T; g.b_clen = Tw; g.tag = "dw_post2";
        WN_TRY(dw_gemm(cs, g, dw_out_plain(grads + y.post2_w, d.S, grads + y.post2_b)));
    }
    if (need_post) {   // d conv_post_1.{weight,bias}
        WnGemmArgs g = wn_gemm_default();
        g.M = d.S; g.N = d.S; g.K = Tw;
        g.A = ws + w.dO2 + t0; g.lda = T; g.a_zstride = (long)d.S * T;
        g.B = ws + w.O1 + t0; g.ldb = T; g.b_zstride = (long)d.S * T; g.b_clen = Tw; g.tag = "dw_post1";
        WN_TRY(dw_gemm(cs, g, dw_out_plain(grads + y.post1_w, d.S, grads + y.post1_b)));
    }
    // Fused skip + res weight gradients (k_dw_skipres: z of every layer read once instead of twice): with the fp16 pair split on,
    // the skip gradients wait for the data chain and are produced per bucket together with the res_1x1 gradients.
    // Only with ONE layer bucket, where the skip weights belong to that bucket (wn_bucket_range); with several, they are part of the
    // head bucket, whose event would then be the last one recorded and hold back the exchange of every layer bucket behind it.
    // And only with launch groups (fmax, below) of at least two layers: the top group's fused launch writes every skip bias, and a
    // top group of the last layer alone ([L-1, L): no res_1x1 gradient) does not take it -- its skip gradients would stay unwritten.
    // Weight gradients are issued for groups of walked layers: a whole bucket in serial mode (largest launches), at
    // most WN_DW_FLUSH_DEFAULT layers in overlap mode so that they start while the chain is still running; flags bits
    // 8..15 override the group size.  (The split-K plan, hence the rounding, depends on the group size.)
    int fmax = (flags >> 8) & 0xff;
    if (fmax == 0) fmax = (side.rt && !(flags & WN_FLAG_BWD_OVERLAP_HEAD)) ? WN_DW_FLUSH_DEFAULT : d.L;
    // (first_layer == L - 1 cuts the top group down to the last layer alone: the same exclusion)
    const bool skipres = c.r.split_bf16 && c.dw_f16_mul != 0.0f && d.L > 1 && lpb >= d.L && fmax >= 2 && fl < d.L - 1 &&
                         wn_dw_skipres_supported(d.S, d.R, d.L, d.L - 1);
    // (over all L layers whenever a layer is computed: the split-K plan, the tile shape and the row sums behind the biases follow
    // the column count, so a contraction over [first_layer, L) alone would not give the computed layers the full pass's bits)
    if (wgrad && !skipres && fl < d.L) {   // d skip_1x1.l.weight for all layers in one contraction; bias = rowsum(dSkip) for every layer
        WnGemmArgs g = wn_gemm_default();
        g.M = d.S; g.N = d.L * d.R; g.K = Tw;
        g.A = ws + w.dSk + t0; g.lda = T; g.a_zstride = (long)d.S * T;
        g.B = ws + w.Z + t0; g.ldb = T; g.b_zstride = (long)d.R * T; g.b_clen = Tw;
        g.b_seg_len = d.R; g.b_seg_stride = w.BRT; g.tag = "dw_skip";
        WN_TRY(dw_gemm(cs, g, dw_out_seg(grads + c.p_skip(0), NO_SEG, 0, d.R, d.R, y.ls_skip, 1, ws + w.tmpS)));
        WN_TRY(skip_bias_all(cs, grads));
    }
    if (events) rt_event_record(events[bucket], cs.st);   // head bucket: the post-net (+ every skip_1x1 with several layer buckets)
    bucket++;

    // ---- residual stack, last layer first (wavenet.py:525-536 reversed) ----
    // The data chain (gate', dX) runs layer by layer; dP_l and dX_l of every layer are kept so that
    // the weight gradients of a whole bucket of layers are produced by ONE launch per tensor kind
    // (layer = outermost z dimension of the dW contraction), then reduced in a fixed order.
    const float* upw = d.U > 0 ? params + y.up_w : ws + w.one;
    const bool aux_fused = c.r.aux_fused, chain = c.r.chain;
    // (all L * R rows whatever first_layer is: the pre-split image of wskipT_f is one [k][rows] block and the kernel variant
    // follows the row count, so a launch over fewer rows would not give the computed layers the full pass's bits)
    if (chain && fl < d.L) {
        WnGemmArgs g = wn_gemm_default();
        g.M = d.L * d.R; g.N = Tw; g.K = d.S;
        g.A = ws + w.wskipT_f; g.lda = (long)d.L * d.R;
        g.B = ws + w.dSk + t0; g.ldb = T; g.b_zstride = (long)d.S * T; g.b_clen = Tw;
        g.C = c.dZs(0) + t0; g.ldc = T; g.c_zstride = c.dZs_B();
        g.nbatch = B; g.tag = "bwd_dz_skip_all";
        WN_TRY(fw_gemm(c, g, nullptr, nullptr, t0, true));
        // dZs[.., t < t0] stays unwritten: the chain kernel takes it as zero without reading it (ChainArgs.zs_t0)
    }
    // WN_FLAG_BWD_OVERLAP_HEAD: only the post-net / skip weight gradients (matrix-bound) go to the side stream, the
    // per-layer groups (HBM-bound like the chain itself) follow the chain on the caller's stream
    const Ctx& cl = (flags & WN_FLAG_BWD_OVERLAP_HEAD) ? c : cs;
    auto flush_bucket = [&](int lo, int hi) -> int {   // every launch of a flush is a weight gradient: on cl
        const int nl = hi - lo;
        const long lb_lo = cl.p_layer(lo);
        float* dc = cl.dc(lo);
        float* dG = cl.dG(dh ? lo : 0);   // dh: every layer's dG stays for the dh launch
        // through the upsampling layer: dG[f] = sum_j w[j] dP[fU+j] of layers [lo, hi), from the gate kernel's partials or from dP
        auto aux_dG = [&]() -> int {
            if (aux_fused)
                return wn_aux_finish(cl.dGp(lo), cl.dGp_L(), cl.qp(lo), cl.qp_L(), dG, cl.dw_partial(lo), B, T, 2 * d.R, Ue, F, nl, cl.st);
            return wn_aux_bwd(cl.P(lo), cl.P_L(), cl.G(lo), cl.G_B(), upw, dG, cl.dw_partial(lo), B, T, 2 * d.R, Ue, F, nl, cl.st);
        };
        if (!wgrad) return d.U > 0 ? aux_dG() : 0;   // dG alone (dh through the upsampling layer); without it dh reads dP
        {   // d dil_{sigmoid,tanh}.l.conv.weight ; dc_l = rowsum(dP_l) -> conv + aux biases
            WnGemmArgs g = wn_gemm_default();
            g.M = 2 * d.R; g.N = d.K * d.R; g.K = T;
            g.A = cl.P(lo); g.lda = T; g.a_zstride = (long)2 * d.R * T; g.a_lstride = cl.P_L();
            g.B = cl.X(lo); g.ldb = T; g.b_zstride = (long)d.R * T; g.b_lstride = w.BRT; g.b_clen = T;
            g.b_seg_len = d.R; g.b_seg_stride = 0; g.b_shift0 = d.K - 1; g.b_shift_step = -1;
            g.b_dil_depth = cfg->dilation_depth; g.b_layer0 = lo;
            g.tag = "dw_dilated";
            DwOut o = dw_out_seg(grads + lb_lo + y.o_dsig_w, d.R, y.o_dtanh_w - y.o_dsig_w, (long)d.R * d.K, d.R, 1, d.K, dc);
            o.out_lstride = -y.LB; o.rowsum_lstride = 2 * d.R;
            WN_TRY(dw_gemm(cl, g, o, nl));
            WnCopy4 cp;  // biases: dil_{sig,tanh}.bias = dc ; aux_{sig,tanh}.bias = dc
            cp.n0 = 1; cp.n1 = 2; cp.n2 = d.R; cp.nl = nl;
            cp.s0 = 0; cp.s1 = d.R; cp.s2 = 1; cp.sl = 2 * d.R;
            cp.d0 = 0; cp.d1 = y.o_dtanh_b - y.o_dsig_b; cp.d2 = 1; cp.dl = -y.LB;
            WN_TRY(wn_copy4(grads + lb_lo + y.o_dsig_b, dc, &cp, cl.st));
            cp.d1 = y.o_atanh_b - y.o_asig_b;
            WN_TRY(wn_copy4(grads + lb_lo + y.o_asig_b, dc, &cp, cl.st));
        }
        const int hi_res = hi < d.L ? hi : d.L - 1;
        const int n_res = hi_res - lo;
        const bool fuse = skipres && n_res > 0;   // (a bucket holding only the last layer has no res_1x1 gradient)
        // the last layer's res_1x1 is dead -> zeros
        if (hi == d.L) WN_TRY(wn_fill(grads + cl.p_layer(d.L - 1) + y.o_res_w, 0.0f, (long)d.R * d.R + d.R, cl.st));
        DwOut o_res = dw_out_plain(grads + lb_lo + y.o_res_w, d.R, grads + lb_lo + y.o_res_b);
        o_res.out_lstride = -y.LB; o_res.rowsum_lstride = -y.LB;
        if (fuse) {
            // skip_1x1 and res_1x1 of layers [lo, hi) against one read of z; the partial sums land where the two separate launches
            // put them, so their conditional six-product launches (same split-K plan) and their reductions follow unchanged
            const DwPlan p = dw_skipres_plan(d.S, nl, T, B);
            WnDwSkipRes a;
            a.S = d.S; a.nl = nl; a.n_res = n_res; a.K = T; a.nbatch = B; a.ksplit = p.ksplit; a.kchunk = p.kchunk;
            a.dS = ws + w.dSk; a.ds_ld = T; a.ds_zstride = (long)d.S * T;
            a.Z = cl.Z(lo); a.z_ld = T; a.z_zstride = (long)d.R * T; a.z_lstride = w.BRT;
            a.dX = cl.dX(lo + 1); a.dx_ld = T; a.dx_zstride = (long)d.R * T; a.dx_lstride = w.BRT;
            a.Cskip = ws + w.partial; a.Cres = ws + w.partial2;
            a.rs_skip = hi == d.L ? ws + w.rs_partial : nullptr;   // rowsum(dSkip): once per step, by the first bucket
            a.rs_res = ws + w.rs_partial2;
            WN_TRY(wn_dw_skipres_launch(&a, cl.dw_f16_mul, cl.dw_ovf, cl.st));
            // the redo launches (no work unless the word is up) and the reductions
            WnGemmArgs gs = wn_gemm_default();
            gs.M = d.S; gs.N = nl * d.R; gs.K = T;
            gs.A = a.dS; gs.lda = T; gs.a_zstride = a.ds_zstride;
            gs.B = a.Z; gs.ldb = T; gs.b_zstride = a.z_zstride; gs.b_clen = T;
            gs.b_seg_len = d.R; gs.b_seg_stride = w.BRT; gs.tag = "dw_skip";
            gs.a_kmajor = 1; gs.b_kmajor = 1; gs.nlayer = 1; gs.nbatch = B; gs.ksplit = p.ksplit; gs.kchunk = p.kchunk;
            gs.C = a.Cskip; gs.ldc = gs.N; gs.c_zstride = (long)gs.M * gs.N;
            gs.a_rowsum = a.rs_skip;
            WN_TRY(wn_gemm6_dw_launch(&gs, 6, 0.0f, cl.dw_ovf, cl.st));
            WnGemmArgs gr = wn_gemm_default();
            gr.M = d.R; gr.N = d.R; gr.K = T;
            gr.A = a.dX; gr.lda = T; gr.a_zstride = a.dx_zstride; gr.a_lstride = w.BRT;
            gr.B = a.Z; gr.ldb = T; gr.b_zstride = a.z_zstride; gr.b_lstride = w.BRT; gr.b_clen = T; gr.tag = "dw_res";
            gr.a_kmajor = 1; gr.b_kmajor = 1; gr.nlayer = n_res; gr.nbatch = B; gr.ksplit = p.ksplit; gr.kchunk = p.kchunk;
            gr.C = a.Cres; gr.ldc = gr.N; gr.c_zstride = (long)gr.M * gr.N;
            gr.a_rowsum = a.rs_res;
            WN_TRY(wn_gemm6_dw_launch(&gr, 6, 0.0f, cl.dw_ovf, cl.st));
            const DwOut o = dw_out_seg(grads + cl.p_skip(lo), NO_SEG, 0, d.R, d.R, y.ls_skip, 1, a.rs_skip ? ws + w.tmpS : nullptr);
            WN_TRY(dw_reduce(cl, a.Cskip, a.rs_skip, p.nz, d.S, nl * d.R, o, 1));
            if (a.rs_skip) WN_TRY(skip_bias_all(cl, grads));
            WN_TRY(dw_reduce(cl, a.Cres, a.rs_res, p.nz, d.R, d.R, o_res, n_res));
        } else if (n_res > 0) {   // d res_1x1.l = dX_{l+1} . z_l^T
            WnGemmArgs g = wn_gemm_default();
            g.M = d.R; g.N = d.R; g.K = T;
            g.A = cl.dX(lo + 1); g.lda = T; g.a_zstride = (long)d.R * T; g.a_lstride = w.BRT;
            g.B = cl.Z(lo); g.ldb = T; g.b_zstride = (long)d.R * T; g.b_lstride = w.BRT; g.b_clen = T;
            g.tag = "dw_res";
            WN_TRY(dw_gemm(cl, g, o_res, n_res));
        }
        {   // d aux_1x1_{sigmoid,tanh}.l.weight
            DwOut o = dw_out_seg(grads + lb_lo + y.o_asig_w, d.R, y.o_atanh_w - y.o_asig_w, d.A, NO_SEG, 0, 1, nullptr);
            o.out_lstride = -y.LB;
            WnGemmArgs g = wn_gemm_default();
            g.tag = "dw_aux";
            g.M = 2 * d.R; g.N = d.A;
            if (d.U > 0) {   // dW = dG.h^T + b_up*dc (x) 1
                WN_TRY(aux_dG());
                g.K = F;
                g.A = dG; g.lda = F; g.a_zstride = (long)2 * d.R * F; g.a_lstride = cl.dG_L();
                g.B = h; g.ldb = F; g.b_zstride = (long)d.A * F; g.b_lstride = 0; g.b_clen = F;
                o.addend_m = dc; o.addend_scale_ptr = params + y.up_b; o.addend_lstride = 2 * d.R;
            } else {
                g.K = T;
                g.A = cl.P(lo); g.lda = T; g.a_zstride = (long)2 * d.R * T; g.a_lstride = cl.P_L();
                g.B = h; g.ldb = T; g.b_zstride = (long)d.A * T; g.b_lstride = 0; g.b_clen = T;
            }
            WN_TRY(dw_gemm(cl, g, o, nl));
        }
        return 0;
    };

    int bucket_hi = d.L;  // layers [l, bucket_hi) have been walked but not flushed yet
    for (int l = d.L - 1; l >= 0; --l) {
        const bool computed = l >= fl;                        // below first_layer: only the bucket bookkeeping
        const bool want_dx = l > fl || (l == 0 && need_front);   // dX_l feeds layer l - 1 (or the front conv): not below the cut
        const int dil = dilation_of(cfg, l);
        const float* Sl = c.Sg(l);
        const float* Gtl = c.Gt(l);   // any-size path only: the fused forward saves s and z = s * tanh
        const float* Zl = c.Z(l);     // second gate operand of the fused kernels: z = s * tanh (g = z / s)
        const int gz = 1;
        float* dP = c.P(l);
        const float* dXn = (l + 1 < d.L) ? c.dX(l + 1) : nullptr;  // null: dead (last layer)
        float* dXl = c.dX(l);
        const float* wskip = params + c.p_skip(l);
        const float* wres = params + c.p_layer(l) + y.o_res_w;
        if (!computed) {
        } else if (chain) {
            if (l == d.L - 1) {   // head of the chain: gate' of the last layer on its rows of dZs (no dX input)
                WN_TRY(wn_fused_bwd_chain_head(c.dZs(l), c.dZs_B(), Sl, Zl, gz, dP, c.G(l), c.G_B(), upw, Ue, F,
                                               aux_fused ? c.dGp(l) : nullptr, aux_fused ? c.qp(l) : nullptr, B, T, t0,
                                               c.r.chain_f16 ? c.amaxP(l) : nullptr, c.st));
            }
            if (l > fl) {  // dX_l from dP_l, and gate' of layer l-1 from it
                const int lp = l - 1;
                WN_TRY(wn_fused_bwd_chain(c.wd_b(l), dP, dXn, dXl, params + c.p_layer(lp) + y.o_res_w, c.dZs(lp), c.dZs_B(),
                                          c.Sg(lp), c.Z(lp), gz, c.P(lp), c.G(lp), c.G_B(), upw, Ue, F,
                                          aux_fused ? c.dGp(lp) : nullptr, aux_fused ? c.qp(lp) : nullptr, B, T, d.K, dil,
                                          c.img(1, l, c.r.chain_f16), c.img(2, lp, c.r.chain_f16), t0,
                                          c.r.chain_f16 ? c.amaxP(l) : nullptr, c.r.chain_f16 ? c.amaxP(lp) : nullptr, c.st));
            } else if (want_dx) {      // tail: dX_0
                WN_TRY(wn_fused_bwd_dx(c.wd_b(0), dP, dXn, dXl, B, T, d.K, dil, 1, c.st));
            }
        } else if (c.r.fused) {
            // dZ = Wskip^T dSk (+ Wres^T dXn) -> gate' -> dP
            if (aux_fused)
                WN_TRY(wn_fused_bwd_gate_aux(wskip, wres, ws + w.dSk, dXn, Sl, Zl, gz, dP, c.G(l), c.G_B(), upw, Ue, F, c.dGp(l),
                                             c.qp(l), B, T, d.S, c.st));
            else
                WN_TRY(wn_fused_bwd_gate(wskip, wres, ws + w.dSk, dXn, Sl, Zl, gz, dP, B, T, d.S, c.r.split_bf16 ? 1 : 0, c.st));
            if (want_dx) WN_TRY(wn_fused_bwd_dx(c.wd_b(l), dP, dXn, dXl, B, T, d.K, dil, c.r.split_bf16 ? 1 : 0, c.st));
        } else {
            // dZ = Wskip_l^T dSkip (+ Wres_l^T dX_{l+1}) -> gate' -> dP.  Wide models on the split kernels: gate' is the
            // epilogue of the LAST of the two contractions (dZ never leaves the chip for it).
            WnGemmArgs gs = wn_gemm_default();
            gs.M = d.R; gs.N = T; gs.K = d.S;
            gs.A = wskip; gs.lda = d.R;
            gs.B = ws + w.dSk; gs.ldb = T; gs.b_zstride = (long)d.S * T; gs.b_clen = T;
            gs.C = ws + w.dZ; gs.ldc = T; gs.c_zstride = (long)d.R * T;
            gs.nbatch = B; gs.tag = "bwd_dz_skip_layered";
            WnGemmArgs gr = wn_gemm_default();
            gr.M = d.R; gr.N = T; gr.K = d.R;
            gr.A = wres; gr.lda = d.R;
            gr.B = dXn; gr.ldb = T; gr.b_zstride = (long)d.R * T; gr.b_clen = T;
            gr.C = ws + w.dZ; gr.ldc = T; gr.c_zstride = (long)d.R * T;
            gr.accumulate = 1; gr.nbatch = B; gr.tag = "bwd_dz_res_layered";
            const bool epi = d.R % 128 == 0 && split_ok(c, gs) && (!dXn || split_ok(c, gr));
            GateEpi ge;
            ge.bw_S = Sl; ge.bw_Gt = Gtl; ge.bw_dP = dP;
            if (epi) {
                if (dXn) {
                    WN_TRY(fw_gemm(c, gs, nullptr, nullptr, 0, true));
                    gr.tag = "bwd_dz_res_gate";
                    WN_TRY(fw_gemm(c, gr, &ge, nullptr, 0, true));
                } else {
                    gs.tag = "bwd_dz_skip_gate";
                    WN_TRY(fw_gemm(c, gs, &ge, nullptr, 0, true));
                }
            } else {
                WN_TRY(fw_gemm(c, gs, nullptr, nullptr, 0, true));
                if (dXn) WN_TRY(fw_gemm(c, gr, nullptr, nullptr, 0, true));
                WN_TRY(wn_gate_bwd(ws + w.dZ, Sl, Gtl, dP, B, T, d.R, c.st));
            }
            if (want_dx) {   // dX_l = dX_{l+1} + sum_tap W_tap^T dP[t + (K-1-tap) d]
                WnGemmArgs g = wn_gemm_default();
                g.M = d.R; g.N = T; g.K = d.K * 2 * d.R;
                g.A = c.wd_b(l); g.lda = d.R;
                g.B = dP; g.ldb = T; g.b_zstride = (long)2 * d.R * T; g.b_clen = T;
                g.b_seg_len = 2 * d.R; g.b_seg_stride = 0; g.b_shift0 = -(d.K - 1) * dil; g.b_shift_step = dil;
                g.C = dXl; g.ldc = T; g.c_zstride = (long)d.R * T;
                if (dXn) { g.D = dXn; g.ldd = T; g.d_zstride = (long)d.R * T; }
                g.nbatch = B; g.tag = "bwd_dx_dilated";
                WN_TRY(fw_gemm(c, g, nullptr, nullptr, 0, true));
            }
        }
        const int done = d.L - l;  // layers walked
        const bool bucket_end = (done % lpb == 0 || l == 0);
        if (bucket_end || bucket_hi - l >= fmax || l == fl) {   // (l == first_layer: the lowest group is cut here)
            if (computed) {
                WN_TRY(side_link(side.rt, c.st, cl.st));  // dP, dX of layers [l, bucket_hi) are enqueued
                if (flags & WN_FLAG_BWD_OVERLAP_HEAD)       // the split-K partial buffers are shared with the head's launches
                    WN_TRY(side_link(side.rt, cs.st, c.st));
                WN_TRY(flush_bucket(l, bucket_hi));
            }
            bucket_hi = l;
            if (bucket_end) {
                if (events) rt_event_record(events[bucket], cl.st);
                bucket++;
            }
        }
    }
    if (dh) {   // dL/dh = sum_l Waux_l^T dG_l (dP_l without the upsampling layer): every layer's operand is final on cl.st
        const int N = d.U > 0 ? F : T;
        // split-K scratch: written and read only here -- dZ (the layered path's per-layer scratch) with the upsampling layer,
        // dG (unused without it) otherwise
        float* scratch = d.U > 0 ? ws + w.dZ : c.dG(0);
        const long scratch_floats = d.U > 0 ? w.BRT : d.L * c.dG_L();
        WN_TRY(wn_aux_dh(ws + w.waux_f, d.A, d.L * 2 * d.R, d.U > 0 ? c.dG(0) : c.P(0), d.U > 0 ? c.dG_L() : c.P_L(),
                         (long)2 * d.R * N, 2 * d.R, N, B, dh, scratch, scratch_floats, cl.st));
    }
    if (!wgrad) {
        WN_TRY(side_link(side.rt, cs.st, c.st));
        return rt_check("wn_backward_dh");
    }
    const float* dXn = c.dX(0);  // dL/dx_0
    // ---- front conv: scatter over the token indices, or (large tables) the one-hot contraction ----
    if (!need_front) {
    } else if (wn_front_dw_supported(d.R, d.K, d.Q) &&
               wn_front_dw_partial_floats(B, T, d.R, d.K, d.Q) <= w.front_partial_floats) {
        WN_TRY(wn_front_dw(dXn, x, ws + w.front_partial, grads + y.causal_w, grads + y.causal_b, B, T, d.R, d.K, d.Q, cl.st));
    } else {
        WnGemmArgs g = wn_gemm_default();
        g.M = d.R; g.N = d.K * d.Q; g.K = T;
        g.A = dXn; g.lda = T; g.a_zstride = (long)d.R * T;
        g.B = ws + w.X; /* unused (b_index set) */ g.ldb = 0; g.b_zstride = 0; g.b_clen = T;
        g.b_seg_len = d.Q; g.b_shift0 = d.K - 1; g.b_shift_step = -1;
        g.b_index = x; g.b_index_zstride = T; g.b_index_mod = d.Q; g.tag = "dw_front_onehot";
        const DwOut o = dw_out_seg(grads + y.causal_w, NO_SEG, 0, (long)d.Q * d.K, d.Q, 1, d.K, grads + y.causal_b);
        WN_TRY(dw_gemm(cl, g, o));
    }
    // ---- upsampling layer parameters ----
    if (d.U > 0 && need_up) {
        WnReduceArgs r = reduce_plain(ws + w.dw_partial, d.L * B * 2 * d.R, 1, d.U, grads + y.up_w, 0, 1);
        r.scratch = ws + w.red_scratch; r.scratch_floats = w.red_scratch_floats;
        WN_TRY(wn_reduce(&r, cl.st));
        // d b_up = sum_{l,o'} rowsum(Waux_l)[o'] * dc_l[o']
        WN_TRY(wn_dot(ws + w.rowsum_aux, ws + w.dc, (long)d.L * 2 * d.R, grads + y.up_b, 0, cl.st));
    }
    if (events) rt_event_record(events[bucket], cl.st);
    bucket++;
    WN_TRY(side_link(side.rt, cs.st, c.st));  // join: the caller's stream continues after every gradient
    return rt_check("wn_backward");
}

extern "C" int wn_backward_window(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                                  const float* dlogits, int t_first, float* grads, void* wsp, size_t ws_bytes,
                                  void* const* events, int n_events, int lpb, int flags, void* stream) {
    api_enter();
    return backward_impl(cfg, B, T, params, x, h, dlogits, t_first, grads, nullptr, wsp, ws_bytes, events, n_events, lpb, flags, stream);
}

extern "C" int wn_backward_dh(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                              const float* dlogits, int t_first, float* grads, float* dh, void* wsp, size_t ws_bytes,
                              void* const* events, int n_events, int lpb, int flags, void* stream) {
    api_enter();
    if (!grads && !dh) return fail(1, "wn_backward_dh: grads and dh are both NULL");
    if (!grads && (events || n_events)) return fail(1, "wn_backward_dh: bucket events need grads (no weight gradients are produced)");
    return backward_impl(cfg, B, T, params, x, h, dlogits, t_first, grads, dh, wsp, ws_bytes, events, n_events, lpb, flags, stream);
}

extern "C" int wn_backward_needs(const WnConfig* cfg, int B, int T, const float* params, const int64_t* x, const float* h,
                                 const float* dlogits, int t_first, float* grads, float* dh, void* wsp, size_t ws_bytes,
                                 void* const* events, int n_events, int lpb, int flags, void* stream, int first_layer, int needs) {
    api_enter();
    if (!grads && !dh) return fail(1, "wn_backward_needs: grads and dh are both NULL");
    if (!grads && (events || n_events)) return fail(1, "wn_backward_needs: bucket events need grads (no weight gradients are produced)");
    return backward_impl(cfg, B, T, params, x, h, dlogits, t_first, grads, dh, wsp, ws_bytes, events, n_events, lpb, flags, stream,
                         first_layer, needs);
}

// ------------------------------------------------------------------------------------------
// What the four Adam entry points ask of the buffers they share (each tests its own step count or state block beside it).
static bool adam_buffers_ok(const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, int64_t n) {
    return params && grads && exp_avg && exp_avg_sq && n > 0;
}

// The bias correction of the host-stepped entry points: lr / bc1 and sqrt(bc2) in double, each rounded to float once
// (k_grad_norm_finalize forms the same two from the device's own count of applied steps).
struct AdamBias {
    float lr_over_bc1, sqrt_bc2;
};
static AdamBias adam_bias(float lr, float beta1, float beta2, int64_t step) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return {(float)((double)lr / bc1), (float)sqrt(bc2)};
}

extern "C" int wn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t step,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int64_t skip_lo,
                            int64_t skip_hi, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || step < 1) return fail(1, "bad wn_adam_step argument");
    const AdamBias b = adam_bias(lr, beta1, beta2, step);
    WN_TRY(wn_adam(params, grads, exp_avg, exp_avg_sq, (long)n, b.lr_over_bc1, b.sqrt_bc2, beta1, beta2, eps, weight_decay,
                   (long)skip_lo, (long)skip_hi, (wn_stream_t)stream));
    return rt_check("wn_adam_step");
}

// ------------------------------------------------------------------------------------------
// Global-norm clipping / non-finite-step guard (ABI v12): the norm (two launches) and the Adam launch that reads its scalars from
// the device state block.  No host synchronisation anywhere.
extern "C" int64_t wn_grad_norm_scratch_floats(int64_t n) {
    return n > 0 ? 2 * (int64_t)wn_grad_sumsq_blocks((long)n) : 0;   // one double per block
}

extern "C" int wn_grad_norm(const float* grads, int64_t n, int64_t skip_lo, int64_t skip_hi, float max_norm, int guard, float lr,
                            float beta1, float beta2, float* scratch, WnOptState* state, void* stream) {
    api_enter();
    if (!grads || !scratch || !state || n <= 0) return fail(1, "bad wn_grad_norm argument");
    if (skip_lo < 0 || skip_hi > n || skip_lo > skip_hi) return fail(1, "wn_grad_norm: skip range outside [0, n]");
    if ((reinterpret_cast<uintptr_t>(grads) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(state) & 7))
        return fail(1, "wn_grad_norm: grads needs 4-byte, scratch and state 8-byte alignment");
    double* partial = reinterpret_cast<double*>(scratch);
    WN_TRY(wn_grad_sumsq(grads, (long)n, (long)skip_lo, (long)skip_hi, partial, (wn_stream_t)stream));
    WN_TRY(wn_grad_norm_finalize(partial, wn_grad_sumsq_blocks((long)n), max_norm, guard != 0, lr, beta1, beta2, state,
                                 (wn_stream_t)stream));
    return rt_check("wn_grad_norm");
}

extern "C" int wn_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float eps,
                                    float weight_decay, int64_t skip_lo, int64_t skip_hi, const WnOptState* state, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || !state) return fail(1, "bad wn_adam_step_guarded argument");
    WN_TRY(wn_adam_guarded(params, grads, exp_avg, exp_avg_sq, (long)n, eps, weight_decay, (long)skip_lo, (long)skip_hi, state,
                           (wn_stream_t)stream));
    return rt_check("wn_adam_step_guarded");
}

// ------------------------------------------------------------------------------------------
// Exponential moving average of the weights in the Adam launch (ABI v14) and the in-place exchange of two buffers.
static bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b), len = (uintptr_t)n * sizeof(float);
    return a0 < b0 + len && b0 < a0 + len;
}

static const char* ema_argument_error(const float* params, const float* ema, int64_t n, double ema_decay) {
    if (!ema) return "ema is NULL";
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return "ema_decay outside [0, 1)";
    if (ranges_overlap(params, ema, n)) return "ema overlaps params";
    return nullptr;
}

extern "C" int wn_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t skip_lo,
                                int64_t skip_hi, double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || step < 1) return fail(1, "bad wn_adam_step_ema argument");
    if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_ema: %s", why);
    const AdamBias b = adam_bias(lr, beta1, beta2, step);
    WN_TRY(wn_adam_ema(params, grads, exp_avg, exp_avg_sq, ema, (long)n, b.lr_over_bc1, b.sqrt_bc2, beta1, beta2, eps, weight_decay,
                       (long)skip_lo, (long)skip_hi, wn_ema_weight(ema_decay, ema_warmup, step), (wn_stream_t)stream));
    return rt_check("wn_adam_step_ema");
}

extern "C" int wn_adam_step_guarded_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                        float eps, float weight_decay, int64_t skip_lo, int64_t skip_hi, const WnOptState* state,
                                        double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || !state) return fail(1, "bad wn_adam_step_guarded_ema argument");
    if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_guarded_ema: %s", why);
    WN_TRY(wn_adam_guarded_ema(params, grads, exp_avg, exp_avg_sq, ema, (long)n, eps, weight_decay, (long)skip_lo, (long)skip_hi,
                               state, ema_decay, ema_warmup, (wn_stream_t)stream));
    return rt_check("wn_adam_step_guarded_ema");
}

// ------------------------------------------------------------------------------------------
// Training with frozen parameters (ABI v16): the norm and the Adam step over live ranges of the flat buffers.  wn_live_table is
// the one place a list of ranges is checked and turned into the table the kernels read; the launching entry points take the
// device copy of what it wrote, with its two host-side facts (n_ranges, n_live).
extern "C" int64_t wn_live_table(const int64_t* ranges, int n_ranges, int64_t n, int64_t* table) {
    g_err[0] = 0;   // pure host code: no runtime call to clear
    if (!ranges || !table) return fail(1, "wn_live_table: NULL argument"), -1;
    if (n_ranges <= 0) return fail(1, "wn_live_table: an empty table (n_ranges = %d)", n_ranges), -1;
    if (n <= 0) return fail(1, "wn_live_table: n <= 0"), -1;
    int64_t before = 0, prev_hi = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const int64_t lo = ranges[2 * r], hi = ranges[2 * r + 1];
        if (lo < 0 || hi > n) return fail(1, "wn_live_table: range %d = [%lld, %lld) outside [0, %lld)", r, (long long)lo, (long long)hi, (long long)n), -1;
        if (hi <= lo) return fail(1, "wn_live_table: range %d = [%lld, %lld) is empty", r, (long long)lo, (long long)hi), -1;
        if (r > 0 && lo < prev_hi) return fail(1, "wn_live_table: range %d = [%lld, %lld) is not behind range %d (the ranges must be sorted and disjoint)", r, (long long)lo, (long long)hi, r - 1), -1;
        table[r] = lo;
        table[n_ranges + r] = hi;
        table[2 * (int64_t)n_ranges + r] = before;
        before += hi - lo;
        prev_hi = hi;
    }
    return before;
}

static const char* live_argument_error(const int64_t* table, int n_ranges, int64_t n_live, int64_t n) {
    if (!table) return "table is NULL";
    if (n_ranges <= 0) return "an empty table";
    if (n_live < n_ranges || n_live > n) return "n_live is not what wn_live_table returned for this table";
    if (reinterpret_cast<uintptr_t>(table) & 7) return "table needs 8-byte alignment";
    return nullptr;
}

extern "C" int wn_grad_norm_live(const float* grads, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, float max_norm,
                                 int guard, float lr, float beta1, float beta2, float* scratch, WnOptState* state, void* stream) {
    api_enter();
    if (!grads || !scratch || !state || n <= 0) return fail(1, "bad wn_grad_norm_live argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_grad_norm_live: %s", why);
    if ((reinterpret_cast<uintptr_t>(grads) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(state) & 7))
        return fail(1, "wn_grad_norm_live: grads needs 4-byte, scratch and state 8-byte alignment");
    double* partial = reinterpret_cast<double*>(scratch);
    WN_TRY(wn_grad_sumsq_live(grads, reinterpret_cast<const long*>(table), n_ranges, (long)n_live, partial, (wn_stream_t)stream));
    WN_TRY(wn_grad_norm_finalize(partial, wn_grad_sumsq_blocks((long)n_live), max_norm, guard != 0, lr, beta1, beta2, state,
                                 (wn_stream_t)stream));
    return rt_check("wn_grad_norm_live");
}

extern "C" int wn_adam_step_live(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                 const int64_t* table, int n_ranges, int64_t n_live, int64_t step, float lr, float beta1, float beta2,
                                 float eps, float weight_decay, double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || step < 1) return fail(1, "bad wn_adam_step_live argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_adam_step_live: %s", why);
    if (ema)
        if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_live: %s", why);
    const AdamBias b = adam_bias(lr, beta1, beta2, step);
    WN_TRY(wn_adam_live(params, grads, exp_avg, exp_avg_sq, ema, reinterpret_cast<const long*>(table), n_ranges, (long)n_live,
                        b.lr_over_bc1, b.sqrt_bc2, beta1, beta2, eps, weight_decay,
                        ema ? wn_ema_weight(ema_decay, ema_warmup, step) : 0.0f, (wn_stream_t)stream));
    return rt_check("wn_adam_step_live");
}

extern "C" int wn_adam_step_guarded_live(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                         const int64_t* table, int n_ranges, int64_t n_live, float eps, float weight_decay,
                                         const WnOptState* state, double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || !state) return fail(1, "bad wn_adam_step_guarded_live argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_adam_step_guarded_live: %s", why);
    if (ema)
        if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_guarded_live: %s", why);
    WN_TRY(wn_adam_guarded_live(params, grads, exp_avg, exp_avg_sq, ema, reinterpret_cast<const long*>(table), n_ranges, (long)n_live,
                                eps, weight_decay, state, ema_decay, ema_warmup, (wn_stream_t)stream));
    return rt_check("wn_adam_step_guarded_live");
}

// ------------------------------------------------------------------------------------------
// Parameter groups (ABI v17): the live table with a group index per range, and the three calls that walk it.  The group values
// are host memory here and launch arguments from here on.
extern "C" int64_t wn_group_table(const int64_t* triples, int n_ranges, int64_t n, int n_groups, int64_t* table) {
    g_err[0] = 0;   // pure host code: no runtime call to clear
    if (!triples || !table) return fail(1, "wn_group_table: NULL argument"), -1;
    if (n_ranges <= 0) return fail(1, "wn_group_table: an empty table (n_ranges = %d)", n_ranges), -1;
    if (n <= 0) return fail(1, "wn_group_table: n <= 0"), -1;
    if (n_groups < 1 || n_groups > WN_MAX_PARAM_GROUPS) return fail(1, "wn_group_table: n_groups = %d outside [1, %d]", n_groups, WN_MAX_PARAM_GROUPS), -1;
    int64_t before = 0, prev_hi = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const int64_t lo = triples[3 * r], hi = triples[3 * r + 1], grp = triples[3 * r + 2];
        if (lo < 0 || hi > n) return fail(1, "wn_group_table: range %d = [%lld, %lld) outside [0, %lld)", r, (long long)lo, (long long)hi, (long long)n), -1;
        if (hi <= lo) return fail(1, "wn_group_table: range %d = [%lld, %lld) is empty", r, (long long)lo, (long long)hi), -1;
        if (r > 0 && lo < prev_hi) return fail(1, "wn_group_table: range %d = [%lld, %lld) is not behind range %d (the ranges must be sorted and disjoint)", r, (long long)lo, (long long)hi, r - 1), -1;
        if (grp < 0 || grp >= n_groups) return fail(1, "wn_group_table: range %d has group %lld outside [0, %d)", r, (long long)grp, n_groups), -1;
        table[r] = lo;
        table[n_ranges + r] = hi;
        table[2 * (int64_t)n_ranges + r] = before;
        table[3 * (int64_t)n_ranges + r] = grp;
        before += hi - lo;
        prev_hi = hi;
    }
    return before;
}

static const char* group_argument_error(const WnAdamGroup* groups, int n_groups) {
    if (!groups) return "groups is NULL";
    if (n_groups < 1 || n_groups > WN_MAX_PARAM_GROUPS) return "n_groups outside [1, WN_MAX_PARAM_GROUPS]";
    return nullptr;
}

static const char* group_block_error(const WnGroupScalars* block) {
    if (!block) return "group_scalars is NULL";
    if (reinterpret_cast<uintptr_t>(block) & 3) return "group_scalars needs 4-byte alignment";
    return nullptr;
}

extern "C" int wn_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                   const int64_t* table, int n_ranges, int64_t n_live, int64_t step, const WnAdamGroup* groups,
                                   int n_groups, float beta1, float beta2, double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || step < 1) return fail(1, "bad wn_adam_step_groups argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_adam_step_groups: %s", why);
    if (const char* why = group_argument_error(groups, n_groups)) return fail(1, "wn_adam_step_groups: %s", why);
    if (ema)
        if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_groups: %s", why);
    // the two double formulas of adam_bias, bc1 kept in double for every group's quotient
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    WnGroupScalars block[WN_MAX_PARAM_GROUPS] = {};
    for (int i = 0; i < n_groups; ++i) block[i] = wn_group_scalars(groups[i], bc1, true);
    WN_TRY(wn_adam_groups(params, grads, exp_avg, exp_avg_sq, ema, reinterpret_cast<const long*>(table), n_ranges, (long)n_live, block,
                          (float)sqrt(bc2), beta1, beta2, ema ? wn_ema_weight(ema_decay, ema_warmup, step) : 0.0f,
                          (wn_stream_t)stream));
    return rt_check("wn_adam_step_groups");
}

extern "C" int wn_grad_norm_groups(const float* grads, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, int64_t skip_lo,
                                   int64_t skip_hi, float max_norm, int guard, const WnAdamGroup* groups, int n_groups, float beta1,
                                   float beta2, float* scratch, WnOptState* state, WnGroupScalars* group_scalars, void* stream) {
    api_enter();
    if (!grads || !scratch || !state || n <= 0) return fail(1, "bad wn_grad_norm_groups argument");
    if (const char* why = group_argument_error(groups, n_groups)) return fail(1, "wn_grad_norm_groups: %s", why);
    if (const char* why = group_block_error(group_scalars)) return fail(1, "wn_grad_norm_groups: %s", why);
    if ((reinterpret_cast<uintptr_t>(grads) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(state) & 7))
        return fail(1, "wn_grad_norm_groups: grads needs 4-byte, scratch and state 8-byte alignment");
    double* partial = reinterpret_cast<double*>(scratch);
    int nb;
    if (table) {
        if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_grad_norm_groups: %s", why);
        if (skip_lo != 0 || skip_hi != 0) return fail(1, "wn_grad_norm_groups: a table and a skip range (the table's ranges say what is read)");
        WN_TRY(wn_grad_sumsq_live(grads, reinterpret_cast<const long*>(table), n_ranges, (long)n_live, partial, (wn_stream_t)stream));
        nb = wn_grad_sumsq_blocks((long)n_live);
    } else {
        if (skip_lo < 0 || skip_hi > n || skip_lo > skip_hi) return fail(1, "wn_grad_norm_groups: skip range outside [0, n]");
        WN_TRY(wn_grad_sumsq(grads, (long)n, (long)skip_lo, (long)skip_hi, partial, (wn_stream_t)stream));
        nb = wn_grad_sumsq_blocks((long)n);
    }
    WN_TRY(wn_grad_norm_finalize_groups(partial, nb, max_norm, guard != 0, groups, n_groups, beta1, beta2, state, group_scalars,
                                        (wn_stream_t)stream));
    return rt_check("wn_grad_norm_groups");
}

extern "C" int wn_adam_step_guarded_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                           const int64_t* table, int n_ranges, int64_t n_live, const WnGroupScalars* group_scalars,
                                           const WnOptState* state, double ema_decay, int ema_warmup, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || !state) return fail(1, "bad wn_adam_step_guarded_groups argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_adam_step_guarded_groups: %s", why);
    if (const char* why = group_block_error(group_scalars)) return fail(1, "wn_adam_step_guarded_groups: %s", why);
    if (ema)
        if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_adam_step_guarded_groups: %s", why);
    WN_TRY(wn_adam_guarded_groups(params, grads, exp_avg, exp_avg_sq, ema, reinterpret_cast<const long*>(table), n_ranges, (long)n_live,
                                  group_scalars, state, ema_decay, ema_warmup, (wn_stream_t)stream));
    return rt_check("wn_adam_step_guarded_groups");
}

// ------------------------------------------------------------------------------------------
// Layer-wise adaptive steps and per-tensor sums of squares (ABI v20): the tensor table -- the group table with one range per
// tensor, an adapt flag and the first block of every range -- and the calls that walk it.
extern "C" int64_t wn_tensor_table(const int64_t* quads, int n_ranges, int64_t n, int n_groups, int64_t* table) {
    g_err[0] = 0;   // pure host code: no runtime call to clear
    if (!quads || !table) return fail(1, "wn_tensor_table: NULL argument"), -1;
    if (n_ranges <= 0) return fail(1, "wn_tensor_table: an empty table (n_ranges = %d)", n_ranges), -1;
    if (n <= 0) return fail(1, "wn_tensor_table: n <= 0"), -1;
    if (n_groups < 1 || n_groups > WN_MAX_PARAM_GROUPS) return fail(1, "wn_tensor_table: n_groups = %d outside [1, %d]", n_groups, WN_MAX_PARAM_GROUPS), -1;
    const int64_t nr = n_ranges;
    int64_t before = 0, prev_hi = 0, blocks = 0;
    for (int r = 0; r < n_ranges; ++r) {
        const int64_t lo = quads[4 * r], hi = quads[4 * r + 1], grp = quads[4 * r + 2], adapt = quads[4 * r + 3];
        if (lo < 0 || hi > n) return fail(1, "wn_tensor_table: range %d = [%lld, %lld) outside [0, %lld)", r, (long long)lo, (long long)hi, (long long)n), -1;
        if (hi <= lo) return fail(1, "wn_tensor_table: range %d = [%lld, %lld) is empty", r, (long long)lo, (long long)hi), -1;
        if (r > 0 && lo < prev_hi) return fail(1, "wn_tensor_table: range %d = [%lld, %lld) is not behind range %d (the ranges must be sorted and disjoint)", r, (long long)lo, (long long)hi, r - 1), -1;
        if (grp < 0 || grp >= n_groups) return fail(1, "wn_tensor_table: range %d has group %lld outside [0, %d)", r, (long long)grp, n_groups), -1;
        if (adapt != 0 && adapt != 1) return fail(1, "wn_tensor_table: range %d has adapt flag %lld (0 or 1)", r, (long long)adapt), -1;
        table[r] = lo;
        table[nr + r] = hi;
        table[2 * nr + r] = before;
        table[3 * nr + r] = grp;
        table[4 * nr + r] = adapt;
        table[5 * nr + r] = blocks;
        before += hi - lo;
        for (int64_t left = hi - lo; left > 0; left -= WN_TENSOR_CHUNK) table[6 * nr + 1 + blocks++] = r;
        prev_hi = hi;
    }
    table[6 * nr] = blocks;
    return before;
}

extern "C" int64_t wn_tensor_blocks(const int64_t* table, int n_ranges) {
    g_err[0] = 0;
    if (!table || n_ranges <= 0) return fail(1, "wn_tensor_blocks: NULL table or n_ranges <= 0"), -1;
    return table[6 * (int64_t)n_ranges];
}

extern "C" int64_t wn_lamb_scratch_floats(int64_t n_blocks) {
    return n_blocks > 0 ? 4 * n_blocks : 0;   // two doubles per block
}

extern "C" int wn_tensor_sumsq(const float* x, int64_t n, const int64_t* table, int n_ranges, int64_t n_live, float* scratch,
                               double* out, void* stream) {
    api_enter();
    if (!x || !scratch || !out || n <= 0) return fail(1, "bad wn_tensor_sumsq argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_tensor_sumsq: %s", why);
    if ((reinterpret_cast<uintptr_t>(x) & 3) || (reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(1, "wn_tensor_sumsq: x needs 4-byte, scratch and out 8-byte alignment");
    WN_TRY(wn_tensor_sumsq_launch(x, reinterpret_cast<const long*>(table), n_ranges, (long)n_live, reinterpret_cast<double*>(scratch),
                                  out, (wn_stream_t)stream));
    return rt_check("wn_tensor_sumsq");
}

extern "C" int wn_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                            const int64_t* table, int n_ranges, int64_t n_live, int64_t step, const WnAdamGroup* groups, int n_groups,
                            float beta1, float beta2, float max_trust, const WnOptState* state, double ema_decay, int ema_warmup,
                            float* scratch, float* stats, void* stream) {
    api_enter();
    if (!adam_buffers_ok(params, grads, exp_avg, exp_avg_sq, n) || (!state && step < 1)) return fail(1, "bad wn_lamb_step argument");
    if (const char* why = live_argument_error(table, n_ranges, n_live, n)) return fail(1, "wn_lamb_step: %s", why);
    if (const char* why = group_argument_error(groups, n_groups)) return fail(1, "wn_lamb_step: %s", why);
    if (ema)
        if (const char* why = ema_argument_error(params, ema, n, ema_decay)) return fail(1, "wn_lamb_step: %s", why);
    if (!(max_trust >= 0.0f)) return fail(1, "wn_lamb_step: max_trust < 0 (0 = no clamp)");
    if (!scratch || !stats) return fail(1, "wn_lamb_step: scratch or stats is NULL");
    if ((reinterpret_cast<uintptr_t>(scratch) & 7) || (reinterpret_cast<uintptr_t>(stats) & 3) || (reinterpret_cast<uintptr_t>(state) & 7))
        return fail(1, "wn_lamb_step: scratch and state need 8-byte, stats 4-byte alignment");
    WN_TRY(wn_lamb(params, grads, exp_avg, exp_avg_sq, ema, reinterpret_cast<const long*>(table), n_ranges, (long)n_live, (long)step,
                   groups, n_groups, beta1, beta2, max_trust, state, ema_decay, ema_warmup, reinterpret_cast<double*>(scratch), stats,
                   (wn_stream_t)stream));
    return rt_check("wn_lamb_step");
}
