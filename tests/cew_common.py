# -*- coding: utf-8 -*-
"""The weighted cross-entropy head (class weights, label smoothing, position weights): checks shared by tests/test_emu_cew.py
(host emulator) and tests/test_gpu_cew.py (MI355X).

Per loss position i, with s the logit column, y the target, p = softmax(s), w the class weights, r the position weights,
W = sum_q w_q:

    ce = -log p_y,   l = (1 - eps) w_y ce + (eps / Q) sum_q w_q (-log p_q)
    g_q = (1 - eps) w_y (p_q - [q == y]) + (eps / Q) (W p_q - w_q)               (dlogits_q * D / (grad_scale * r_i))
    D = sum_i r_i w_{y_i} ("weights") or N ("positions");  loss = (sum r l / D, sum ce / N, D)

References: fp64, from the fp32 inputs the kernel sees.  Yardstick for what fp32 can do: the same formulas by torch on the CPU in
fp32 (``log_softmax(v - v.amax(1, keepdim=True), 1)``) -- the convention of tests/loss_common.py, whose factor 4 and 8 u terms
these gates take over (u = 2^-24); none was fitted to the kernel:

    dlogits, per live position with r > 0   max_q |g_k - g_64|  <=  4 E32 + 8 u ((1 - eps) w_y + eps W / Q)
    pos_loss / r, likewise                  |l_k - l_64|        <=  4 e32 + 8 u max(1, |l_64|)
    loss[0], loss[1]                        the sum of the per-position bounds + 2^-22 sum |.|, over D resp. N  (check_mean's form)
    loss[2]                                 |D_k - D_64| <= 2^-22 D_64

The r == indicator invariant is stated for ``normalize="weights"``: under "positions" the two calls differ in N by definition."""
import ctypes
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import freeze_common as FC
from tests import loss_common as LC
from tests import parity_common as PC

U24 = LC.U24
FACTOR = LC.FACTOR
OP_B, OP_T, OP_T_START, OP_GRAD_SCALE = LC.OP_B, LC.OP_T, LC.OP_T_START, LC.OP_GRAD_SCALE
OP_LENGTHS = LC.OP_LENGTHS
OP_Q = (37, 64, 256, 300)          # a ragged quarter per wave, the plain case, the full register-resident case, the wide route
EPS = 0.1
OPTIONS = {"w": (True, 0.0, False), "eps": (False, EPS, False), "r": (False, 0.0, True), "all": (True, EPS, True)}
NORMALIZE = ("weights", "positions")
OP_MODES = ("dense", "ragged")
OP_MATRIX = [(Q, o, n) for Q in OP_Q for o in OPTIONS for n in NORMALIZE]
# the emulator's subset: every Q, every option, both normalizations, dense and ragged
EMU_MATRIX = [(37, "all", "weights", ("dense", "ragged")), (37, "eps", "positions", ("ragged",)), (64, "w", "weights", ("ragged",)),
              (64, "r", "positions", ("dense",)), (256, "all", "positions", ("ragged",)), (256, "r", "weights", ("dense",)),
              (300, "all", "weights", ("ragged",)), (300, "w", "positions", ("dense",)), (300, "eps", "weights", ("dense",))]
assert {m[0] for m in EMU_MATRIX} == set(OP_Q) and {m[1] for m in EMU_MATRIX} == set(OPTIONS)
PATTERNS = [p for p in LC.PATTERNS if p[0] != "P4"]
assert OP_T - 256 >= len(PATTERNS)   # every pattern also lands in the ragged last block


def _formulas(s, tq, hot, w, eps):
    """The definition in the dtype of s: per position ce, l, w_y (B, T), per class g (B, Q, T), and W.  ``w`` (Q,) or None."""
    Q = s.shape[1]
    logp = torch.log_softmax(s - s.amax(1, keepdim=True), 1)
    p = torch.exp(logp)
    ce = -logp.gather(1, tq[:, None, :])[:, 0]
    wv = torch.ones(Q, dtype=s.dtype) if w is None else w.to(s.dtype)
    wy, W, wq = wv[tq], wv.sum(), wv[None, :, None]
    l = ((1.0 - eps) * wy) * ce
    g = ((1.0 - eps) * wy)[:, None, :] * (p - hot.to(s.dtype))
    if eps != 0.0:
        l = l + (eps / Q) * torch.where(wq > 0, wq * (-logp), torch.zeros_like(logp)).sum(1)
        g = g + (eps / Q) * (W * p - wq)
    return ce, l, g, wy, W


def cew_refs(s32, target, w, eps):
    B, Q, T = s32.shape
    tq = torch.remainder(target, Q)
    hot = torch.zeros((B, Q, T), dtype=torch.bool).scatter_(1, tq[:, None, :], True)
    ce, l, g, wy, W = _formulas(s32.double(), tq, hot, w, eps)
    ce32, l32, g32, _, _ = _formulas(s32, tq, hot, w, eps)
    r = dict(tq=tq, hot=hot, ce=ce, l=l, g=g, wy=wy, W=float(W), eps=eps, Q=Q)
    r["E_g"] = (g32.double() - g).abs().amax(1)
    for k, a32, a in (("ce", ce32, ce), ("l", l32, l)):
        r["e_" + k] = torch.where(torch.isfinite(a), (a32.double() - a).abs(), torch.zeros_like(a))
    return r


def divisor(ref, live, r, normalize):
    """D in fp64 and N."""
    n = int(live.sum())
    if normalize == "positions":
        return float(n), n
    rr = torch.ones_like(ref["wy"]) if r is None else r.double()
    return float((rr * ref["wy"])[live].sum()), n


def pos_bound(ref, what):
    v = ref[what]
    b = FACTOR * ref["e_" + what] + 8 * U24 * v.abs().clamp(min=1.0)
    return torch.where(torch.isfinite(v), b, torch.full_like(b, float("inf")))


def _on(live, r):
    return live if r is None else live & (r > 0)


def check_grad(tag, dk, ref, live, r, D, gs, fam):
    """Exact zeros off the live positions and where r == 0; the per-position gate on dlogits * D / (grad_scale * r_i)."""
    dk = dk.cpu()
    on = _on(live, r)
    off = ~on[:, None, :].expand_as(dk)
    if bool(off.any()):
        assert float(dk[off].abs().max()) == 0.0, tag
    rr = torch.ones_like(ref["wy"]) if r is None else r.double()
    unit = torch.where(on, gs * rr / D, torch.ones_like(rr))
    err = (dk.double() / unit[:, None, :] - ref["g"]).abs().amax(1)
    gate = FACTOR * ref["E_g"] + 8 * U24 * ((1.0 - ref["eps"]) * ref["wy"] + ref["eps"] * ref["W"] / ref["Q"])
    frac = torch.where(on & (gate > 0), err / gate.clamp(min=1e-300), torch.zeros_like(err))
    b, t = divmod(int(frac.argmax()), frac.shape[1])
    print("FIGURE %s dlogits: worst of-gate %.3g at b=%d t=%d %s (err %.3g, torch fp32 %.3g)"
          % (tag, float(frac[b, t]), b, t, fam[t], float(err[b, t]), float(ref["E_g"][b, t])))
    bad = ["%s b=%d t=%d %s: |g_k - g_64| = %.3g > %.3g" % (tag, b, t, fam[t], float(err[b, t]), float(gate[b, t]))
           for b in range(err.shape[0]) for t in range(err.shape[1]) if bool(on[b, t]) and not float(err[b, t]) <= float(gate[b, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])


def check_pos(tag, pos, ref, live, r, fam):
    pos = pos.cpu().double()
    on = _on(live, r)
    if bool((~on).any()):
        assert float(pos[~on].abs().max()) == 0.0, tag
    rr = torch.ones_like(pos) if r is None else torch.where(on, r.double(), torch.ones_like(pos))
    err, gate = (pos / rr - ref["l"]).abs(), pos_bound(ref, "l")
    frac = torch.where(on, err / gate, torch.zeros_like(err))
    b, t = divmod(int(frac.argmax()), frac.shape[1])
    print("FIGURE %s pos_loss: worst of-gate %.3g at b=%d t=%d %s (err %.3g, torch fp32 %.3g)"
          % (tag, float(frac[b, t]), b, t, fam[t], float(err[b, t]), float(ref["e_l"][b, t])))
    bad = ["%s b=%d t=%d %s: |l_k - l_64| = %.3g > %.3g (l_64 = %.9g)" % (tag, b, t, fam[t], float(err[b, t]), float(gate[b, t]), float(ref["l"][b, t]))
           for b in range(err.shape[0]) for t in range(err.shape[1]) if bool(on[b, t]) and not float(err[b, t]) <= float(gate[b, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])


def check_losses(tag, loss3, ref, live, r, D, n):
    """loss[0] and loss[1] in check_mean's form, loss[2] against the fp64 divisor."""
    got = [float(v) for v in loss3.cpu()]
    rr = torch.ones_like(ref["l"]) if r is None else r.double()
    on = _on(live, r)
    want0 = float((rr * ref["l"])[on].sum()) / D
    bound0 = (float((rr * pos_bound(ref, "l"))[on].sum()) + 2.0 ** -22 * float((rr * ref["l"])[on].abs().sum())) / D
    want1 = float(ref["ce"][live].sum()) / n
    bound1 = (float(pos_bound(ref, "ce")[live].sum()) + 2.0 ** -22 * float(ref["ce"][live].abs().sum())) / n
    for i, want, bound in ((0, want0, bound0), (1, want1, bound1), (2, D, 2.0 ** -22 * D)):
        print("FIGURE %s loss[%d]: %.9g, fp64 %.9g, err %.3g (bound %.3g)" % (tag, i, got[i], want, abs(got[i] - want), bound))
        assert abs(got[i] - want) <= bound, (tag, i, got[i], want, abs(got[i] - want), bound)


@functools.lru_cache(maxsize=None)
def op_inputs(Q):
    """(logits (B, Q, T), target (B, T), class weights (Q,), position weights (B, T), family per t): position t carries pattern
    t % len(PATTERNS).  The weights lie in [0.25, 4] but for one class of weight exactly 0, which is the target of a position live
    in every mode; the position weights in [0, 2] with exact zeros on every fifth position."""
    B, T = OP_B, OP_T
    rs = np.random.RandomState(9000 + Q)
    v = np.zeros((B, Q, T), dtype=np.float32)
    tg = np.zeros((B, T), dtype=np.int64)
    for t in range(T):
        _, gen = PATTERNS[t % len(PATTERNS)]
        for b in range(B):
            col, tq = gen(rs, Q, int(rs.randint(Q)))
            v[b, :, t] = col.astype(np.float32)
            tg[b, t] = tq + Q * int(rs.randint(-2, 3))       # modulo Q
    w = rs.uniform(0.25, 4.0, Q).astype(np.float32)
    w[int(tg[0, OP_T_START + 2]) % Q] = 0.0
    r = rs.uniform(0.0, 2.0, (B, T)).astype(np.float32)
    r[:, 3::5] = 0.0
    fam = [PATTERNS[t % len(PATTERNS)][0] for t in range(T)]
    return torch.from_numpy(v), torch.from_numpy(tg), torch.from_numpy(w), torch.from_numpy(r), fam


@functools.lru_cache(maxsize=None)
def op_refs(Q, with_w, eps):
    s, t, w, _, _ = op_inputs(Q)
    return cew_refs(s, t, w if with_w else None, eps)


def self_check():
    """The inputs of the main matrix give finite fp64 references on every position, the zero-weight class is a live target and
    some live position weights are exactly zero."""
    for Q in OP_Q:
        s, t, w, r, _ = op_inputs(Q)
        live = LC.live_mask(OP_B, OP_T, OP_T_START, list(OP_LENGTHS))
        assert float(w.min()) == 0.0 and int((w == 0).sum()) == 1 and float(w[w > 0].min()) >= 0.25 and float(w.max()) <= 4.0
        assert bool((w[torch.remainder(t, Q)][live] == 0).any())
        assert bool((r[live] == 0).any()) and float(r.min()) == 0.0 and float(r.max()) <= 2.0
        for with_w, eps, _ in OPTIONS.values():
            ref = op_refs(Q, with_w, eps)
            for k in ("ce", "l", "g"):
                assert bool(torch.isfinite(ref[k]).all()), (Q, k)


def op_engine(Q, lib, device):
    return WaveNetEngine(Q, *LC.OP_CFG_TAIL, device=device, library=lib)


def _b(t):
    return t.detach().cpu().clone().contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_b(x), _b(y)) for x, y in zip(a, b))


def check_cew_op(Q, option, normalize, modes, lib, device):
    with_w, eps, with_r = OPTIONS[option]
    s32, target, w32, r32, fam = op_inputs(Q)
    ref = op_refs(Q, with_w, eps)
    w, r = (w32 if with_w else None), (r32 if with_r else None)
    B, T, ts, gs = OP_B, OP_T, OP_T_START, OP_GRAD_SCALE
    eng = op_engine(Q, lib, device)
    sd, td = s32.to(device), target.to(device)
    wd, rd = (None if w is None else w.to(device)), (None if r is None else r.to(device))

    def call(lengths=None, cw=wd, pw=rd, norm=normalize, **kw):
        return eng.weighted_loss(sd, td, cw, eps, pw, norm, t_start=ts, grad_scale=gs, lengths=lengths, **kw)

    for name in modes:
        lengths = {"dense": None, "ragged": list(OP_LENGTHS)}[name]
        live = LC.live_mask(B, T, ts, lengths)
        D, n = divisor(ref, live, r, normalize)
        tag = "cew Q=%d %s %s %s" % (Q, option, normalize, name)
        out = call(lengths, want_pos=True)
        loss3, dl, pos = out
        # bit-level invariants: without the gradient and the per-position loss; NaN, then zeros, in scratch and workspace
        l0, none = call(lengths, want_grad=False)
        assert none is None and torch.equal(_b(l0), _b(loss3)), tag
        for fill in (float("nan"), 0.0):
            eng._cew_scratch.fill_(fill)
            eng.workspace(B, T).fill_(fill)
            assert _same(out, call(lengths, want_pos=True)), (tag, fill)
        if name == "dense":   # the ragged entry with full lengths
            assert _same(out, call([T] * B, want_pos=True)), tag
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pos).all()), tag
        check_grad(tag, dl, ref, live, r, D, gs, fam)
        check_pos(tag, pos, ref, live, r, fam)
        check_losses(tag, loss3, ref, live, r, D, n)
        if normalize == "weights":
            if with_w:   # 4 w: the divisor takes the factor back, bit for bit
                l4, d4, p4 = call(lengths, cw=(4.0 * w).to(device), want_pos=True)
                assert torch.equal(_b(l4[0:2]), _b(loss3[0:2])), (tag, l4.cpu(), loss3.cpu())
                assert torch.equal(_b(d4), _b(dl)), tag
                assert float(l4[2].cpu()) == 4.0 * float(loss3[2].cpu()), tag
            if name == "ragged":   # the mask as position weights on a dense call: dead positions add exact zeros
                ind = live.float() if r is None else torch.where(live, r, torch.zeros_like(r))
                li, di, pi = call(None, pw=ind.to(device), want_pos=True)
                assert torch.equal(_b(li[0]), _b(loss3[0])) and torch.equal(_b(li[2]), _b(loss3[2])), tag
                assert torch.equal(_b(di), _b(dl)) and torch.equal(_b(pi), _b(pos)), tag
        # D == 0: zeros where torch gives NaN
        lz, dz, pz = call(lengths, pw=torch.zeros((B, T)).to(device), want_pos=True)
        assert float(dz.abs().max().cpu()) == 0.0 and float(pz.abs().max().cpu()) == 0.0 and float(lz[0].cpu()) == 0.0, tag
        assert torch.equal(_b(lz[1]), _b(loss3[1])), tag
        if normalize == "weights":
            assert float(lz[2].cpu()) == 0.0, tag
            lz, dz = call(lengths, cw=torch.zeros(Q).to(device))
            assert float(dz.abs().max().cpu()) == 0.0 and float(lz[0].cpu()) == 0.0 and float(lz[2].cpu()) == 0.0, tag


def check_cew_torch(Q, lib, device):
    """With r = 1 and normalize = "weights": loss[0] and dlogits against F.cross_entropy(weight=, label_smoothing=) and its
    autograd in fp64, inside the bounds of the per-position checks."""
    s32, target, w32, _, fam = op_inputs(Q)
    B, T, ts, gs = OP_B, OP_T, OP_T_START, OP_GRAD_SCALE
    eng = op_engine(Q, lib, device)
    for with_w, eps in ((True, 0.0), (False, EPS), (True, EPS)):
        w = w32 if with_w else None
        ref = op_refs(Q, with_w, eps)
        for lengths in (None, list(OP_LENGTHS)):
            live = LC.live_mask(B, T, ts, lengths)
            tag = "cew vs torch Q=%d w=%s eps=%g %s" % (Q, with_w, eps, "dense" if lengths is None else "ragged")
            leaf = s32.double().requires_grad_(True)
            cols = leaf.permute(0, 2, 1)[live]                          # (N, Q)
            want = F.cross_entropy(cols, torch.remainder(target, Q)[live], weight=None if w is None else w.double(), label_smoothing=eps)
            want.backward()
            want = want.detach()
            D, n = divisor(ref, live, None, "weights")
            # torch's own value and gradient are the definition's: the fp64 references the gates are built on
            assert abs(float(want) - float(ref["l"][live].sum()) / D) <= 1e-12 * max(1.0, abs(float(want))), tag
            assert float((leaf.grad * D - torch.where(live[:, None, :], ref["g"], torch.zeros_like(ref["g"]))).abs().max()) <= 1e-12 * max(1.0, ref["W"]), tag
            loss3, dl, pos = eng.weighted_loss(s32.to(device), target.to(device), None if w is None else w.to(device), eps, None, "weights",
                                               t_start=ts, grad_scale=gs, lengths=lengths, want_pos=True)
            tref = dict(ref, g=leaf.grad * D)
            check_grad(tag, dl, tref, live, None, D, gs, fam)
            bound = (float(pos_bound(ref, "l")[live].sum()) + 2.0 ** -22 * float(ref["l"][live].abs().sum())) / D
            got = float(loss3[0].cpu())
            print("FIGURE %s loss[0]: %.9g, torch fp64 %.9g, err %.3g (bound %.3g)" % (tag, got, float(want), abs(got - float(want)), bound))
            assert abs(got - float(want)) <= bound, tag


SMALL_T = LC.SMALL_T
MASK_Q = (37, 256, 300)
MASKED = (1, 9, 20)


def _small(Q, seed):
    rs = np.random.RandomState(seed)
    s = torch.from_numpy(rs.standard_normal((1, Q, SMALL_T)).astype(np.float32))
    t = torch.from_numpy(rs.randint(0, Q, size=(1, SMALL_T)).astype(np.int64))
    for q in MASKED:   # the targets stay off the classes the cases mask
        t[t == q] = q + 1
    w = torch.from_numpy(rs.uniform(0.25, 4.0, Q).astype(np.float32))
    r = torch.from_numpy(rs.uniform(0.5, 2.0, (1, SMALL_T)).astype(np.float32))
    return s, t, w, r


def check_cew_masked(Q, lib, device):
    eng = op_engine(Q, lib, device)
    s, t, w, r = _small(Q, 9100 + Q)
    live = LC.live_mask(1, SMALL_T, 0)
    fam = ["M"] * SMALL_T
    w0 = w.clone()
    w0[list(MASKED)] = 0.0
    for fill in (-float("inf"), -1e30):
        sm = s.clone()
        sm[0, list(MASKED), :] = fill
        # a masked class of weight 0 under smoothing, and any masked class without smoothing, adds exactly 0: everything finite
        for wv, eps in ((w0, EPS), (w, 0.0)):
            for norm in NORMALIZE:
                ref = cew_refs(sm, t, wv, eps)
                D, n = divisor(ref, live, r, norm)
                tag = "cew Q=%d masked %g eps=%g %s" % (Q, fill, eps, norm)
                loss3, dl, pos = eng.weighted_loss(sm.to(device), t.to(device), wv.to(device), eps, r.to(device), norm, t_start=0,
                                                   want_pos=True)
                assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pos).all()), tag
                assert float(dl.cpu()[0, list(MASKED), :].abs().max()) == 0.0, tag
                check_grad(tag, dl, ref, live, r, D, 1.0, fam)
                check_pos(tag, pos, ref, live, r, fam)
                check_losses(tag, loss3, ref, live, r, D, n)
    # smoothing with a positive weight on a class at -inf: +inf as torch gives, in that position alone; the gradient is finite
    sm = s.clone()
    sm[0, MASKED[0], 3] = -float("inf")
    ref = cew_refs(sm, t, w, EPS)
    tq = torch.remainder(t, Q)
    l32 = _formulas(sm, tq, ref["hot"], w, EPS)[1]
    assert float(l32[0, 3]) == float("inf") and float(F.cross_entropy(sm[0].t(), t[0], weight=w, label_smoothing=EPS)) == float("inf")
    D, n = divisor(ref, live, r, "weights")
    loss3, dl, pos = eng.weighted_loss(sm.to(device), t.to(device), w.to(device), EPS, r.to(device), "weights", t_start=0, want_pos=True)
    l = [float(v) for v in loss3.cpu()]
    assert l[0] == float("inf") and math.isfinite(l[1]) and math.isfinite(l[2]), l
    assert bool(torch.isfinite(dl).all())
    assert float(pos.cpu()[0, 3]) == float("inf") and bool(torch.isfinite(pos.cpu()[0, [c for c in range(SMALL_T) if c != 3]]).all())
    check_grad("cew Q=%d smoothing onto -inf" % Q, dl, ref, live, r, D, 1.0, fam)


def check_cew_nonfinite(Q, lib, device):
    """One NaN, and in another call one +inf, in one column: the criterion, that column's ``dlogits`` and its ``pos_loss`` are
    non-finite, every other column has the bits of the clean call."""
    eng = op_engine(Q, lib, device)
    s, t, w, r = _small(Q, 9200 + Q)
    col = 3
    keep = [c for c in range(SMALL_T) if c != col]
    for wv, eps, rv, norm in ((w, 0.0, None, "weights"), (w, EPS, r, "weights"), (None, EPS, r, "positions")):
        args = (None if wv is None else wv.to(device), eps, None if rv is None else rv.to(device), norm)
        _, base, pbase = eng.weighted_loss(s.to(device), t.to(device), *args, t_start=0, want_pos=True)
        base, pbase = base.cpu().clone(), pbase.cpu().clone()
        for bad in (float("nan"), float("inf")):
            sb = s.clone()
            sb[0, (int(t[0, col]) + 1) % Q, col] = bad
            loss3, dl, pos = eng.weighted_loss(sb.to(device), t.to(device), *args, t_start=0, want_pos=True)
            dl, pos = dl.cpu(), pos.cpu()
            assert not math.isfinite(float(loss3[0].cpu())), (bad, eps)
            assert not bool(torch.isfinite(dl[0, :, col]).any()), (bad, eps, dl[0, :, col])
            assert not math.isfinite(float(pos[0, col])), (bad, eps)
            assert torch.equal(_b(dl[:, :, keep]), _b(base[:, :, keep])) and torch.equal(_b(pos[:, keep]), _b(pbase[:, keep])), (bad, eps)


def check_cew_errors(lib, device):
    """Every refusal of the C entry and of the Python keywords: an error, and nothing launched."""
    Q, B, T = 37, 1, SMALL_T
    eng = op_engine(Q, lib, device)
    s, t, w, r = (a.to(device) for a in _small(Q, 9300))
    ws = eng.workspace(B, T)
    loss = torch.zeros(3, dtype=torch.float32, device=device)
    n_scr = int(eng.lib.wn_softmax_cew_scratch_floats(B, T))
    scratch = torch.zeros(n_scr + 2, dtype=torch.float32, device=device)
    assert n_scr >= 2 * 3 + 3 and eng.lib.wn_softmax_cew_scratch_floats(2, 304) >= 2 * (2 + 2) + 3 * 2 * 5
    assert eng.lib.wn_softmax_cew_scratch_floats(0, 8) == 0

    def call(cfg=None, logits=s, target=t, t_start=0, n_loss=B * T, cw=w, pw=r, eps=0.1, norm=0, out=loss, scr=scratch):
        return eng.lib.wn_softmax_cew_loss(ctypes.byref(cfg or eng.cfg), B, T, _ptr(logits), _ptr(target), t_start, None, n_loss,
                                           _ptr(cw), _ptr(pw), eps, norm, 1.0, 1.0, _ptr(out), None, None, _ptr(scr), _ptr(ws),
                                           ws.numel() * 4, _stream_handle(eng.device))

    assert call() == 0, eng.lib.wn_last_error().decode()
    assert call(cw=None, pw=None, eps=0.0, norm=1) == 0, eng.lib.wn_last_error().decode()
    for kw, word in ((dict(eps=-0.1), "eps"), (dict(eps=1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(norm=2), "normalize"),
                     (dict(norm=-1), "normalize"), (dict(logits=None), "logits"), (dict(target=None), "target"), (dict(out=None), "loss"),
                     (dict(scr=None), "scratch"), (dict(scr=scratch[1:]), "aligned"), (dict(n_loss=0), "n_loss"),
                     (dict(n_loss=B * T - 1), "n_loss"), (dict(t_start=T), "t_start")):
        loss.fill_(7.0)
        rc = []
        log = PC.launch_log(eng.lib, lambda: rc.append(call(**kw)))
        assert rc[0] != 0 and not log, (kw, log)
        msg = eng.lib.wn_last_error().decode()
        assert word in msg, (kw, msg)
        if "out" not in kw:
            assert float(loss.cpu()[0]) == 7.0, kw   # an error code, never a launch
    mol = WaveNetEngine(Q, *LC.OP_CFG_TAIL, device=device, library=lib, out_channels=3 * 4)
    wsm = mol.workspace(B, T)
    rc = mol.lib.wn_softmax_cew_loss(ctypes.byref(mol.cfg), B, T, _ptr(s), _ptr(t), 0, None, B * T, None, None, 0.1, 0, 1.0, 1.0,
                                     _ptr(loss), None, None, _ptr(scratch), _ptr(wsm), wsm.numel() * 4, _stream_handle(mol.device))
    assert rc != 0 and "out_channels" in mol.lib.wn_last_error().decode()
    # the engine's keywords
    host_w = w.cpu()
    for kw, word in ((dict(label_smoothing=1.0), "label_smoothing"), (dict(label_smoothing=-0.5), "label_smoothing"),
                     (dict(normalize="mean"), "normalize"), (dict(class_weights=host_w[:-1]), "class_weights"),
                     (dict(class_weights=host_w.double()), "class_weights"), (dict(class_weights=-host_w), "class_weights"),
                     (dict(class_weights=host_w * float("inf")), "class_weights"),
                     (dict(position_weights=torch.ones(B, T + 1)), "position_weights"),
                     (dict(position_weights=torch.full((B, T), float("nan"))), "position_weights")):
        def bad():
            try:
                eng.weighted_loss(s, t, t_start=0, **kw)
            except ValueError as e:
                assert word in str(e), (kw, str(e))
            else:
                raise AssertionError("weighted_loss took %r" % (kw,))
        assert not PC.launch_log(eng.lib, bad), kw
    try:
        mol.weighted_loss(s, t, label_smoothing=0.1)
    except ValueError as e:
        assert "softmax head" in str(e)
    else:
        raise AssertionError("a mixture-head engine took weighted_loss")
    # a host weight tensor is checked once: the second call with the same object makes no new device copy
    eng.weighted_loss(s, t, class_weights=host_w, t_start=0)
    first = eng._weights_seen["class_weights"][2]
    eng.weighted_loss(s, t, class_weights=host_w, t_start=0)
    assert eng._weights_seen["class_weights"][2] is first
    host_w[0] = -1.0   # (an in-place change is a new version: checked again)
    try:
        eng.weighted_loss(s, t, class_weights=host_w, t_start=0)
    except ValueError:
        pass
    else:
        raise AssertionError("a changed weight tensor was not checked again")


# ---------------------------------------------------------------------------------------------------------------------
# model level: WaveNet.loss_and_backward(class_weights=, label_smoothing=, position_weights=, normalize=)
# ---------------------------------------------------------------------------------------------------------------------
MODEL = (128, 4, 64, 128, 2, 1, 2, 0)
M_B, M_T = 2, 272
M_LENGTHS = (150, M_T)
M_EPS = 0.1


@functools.lru_cache(maxsize=None)
def model_instance():
    cfg = O.OracleConfig(*MODEL)
    params, x, h, t, _, _ = PC.pick_instance(cfg, M_B, M_T, 9400, 0.3)
    rs = np.random.RandomState(9401)
    w = torch.from_numpy(rs.uniform(0.25, 4.0, MODEL[0]).astype(np.float32))
    w[int(t[0, cfg.receptive_field + 1])] = 0.0
    r = torch.from_numpy(rs.uniform(0.0, 2.0, (M_B, M_T)).astype(np.float32))
    r[:, 3::5] = 0.0
    return cfg, params, x, h, t, w, r


def _model(lib, dev):
    cfg, params, x, h, t, w, r = model_instance()
    model = WaveNet(*MODEL, _library=lib)
    model.load_state_dict(params)
    model.to(dev)
    return model, x.to(dev), h.to(dev), t.to(dev), w.to(dev), r.to(dev), cfg.receptive_field


def _by_hand(model, xd, hd, td, opts, t_start, grad_scale=1.0, lengths=None, dh=None, **needs):
    eng = model.engine
    logits = eng.forward(xd, hd)
    loss3, dl = eng.weighted_loss(logits, td, t_start=t_start, grad_scale=grad_scale, lengths=lengths, **opts)
    flat = eng.backward(dl, t_first=t_start, dh=dh, **needs)
    return _b(loss3), _b(flat)


def check_model_composition(lib, dev, option_sets=3):
    """``option_sets``: how many of the three keyword sets run (the host emulator takes the first, the one with every option)."""
    model, xd, hd, td, wd, rd, ts = _model(lib, dev)
    eng = model.engine
    for opts in (dict(class_weights=wd, label_smoothing=M_EPS, position_weights=rd, normalize="weights"),
                 dict(label_smoothing=M_EPS, normalize="positions"), dict(position_weights=rd))[:option_sets]:
        for lengths in (None, list(M_LENGTHS)):
            l3, g = _by_hand(model, xd, hd, td, opts, ts, lengths=lengths)
            eng.grads().fill_(float("nan"))
            loss = model.loss_and_backward(xd, hd, td, lengths=lengths, **opts)
            assert tuple(loss.shape) == (1,) and torch.equal(_b(loss), l3[0:1]) and torch.equal(_b(model.criterion_parts), l3)
            assert torch.equal(_b(eng.grads()), g), (sorted(opts), lengths)
            # aux_grad: the same dh
            dh0 = torch.empty_like(hd)
            _, g2 = _by_hand(model, xd, hd, td, opts, ts, lengths=lengths, dh=dh0)
            loss, dh = model.loss_and_backward(xd, hd, td, lengths=lengths, aux_grad=True, **opts)
            assert torch.equal(_b(dh), _b(dh0)) and torch.equal(_b(eng.grads()), g2) and torch.equal(_b(loss), l3[0:1])
    # two micro-steps: the sum of the hand-composed halves
    opts = dict(class_weights=wd, label_smoothing=M_EPS, position_weights=rd, normalize="positions")
    _, ga = _by_hand(model, xd, hd, td, opts, ts, grad_scale=0.5)
    _, gb = _by_hand(model, xd, hd, td, opts, ts, grad_scale=0.5, lengths=list(M_LENGTHS))
    model.loss_and_backward(xd, hd, td, grad_scale=0.5, micro_step=(0, 2), **opts)
    model.loss_and_backward(xd, hd, td, grad_scale=0.5, lengths=list(M_LENGTHS), micro_step=(1, 2), **opts)
    assert torch.equal(_b(eng.grads()), _b(ga.view(torch.float32) + gb.view(torch.float32)))
    # the refusals of the keywords launch nothing and open no accumulation cycle
    mol = WaveNet(*MODEL, n_mixture=2, _library=lib).to(dev)
    tl = torch.zeros((M_B, MODEL[0], M_T), dtype=torch.float32, device=xd.device)
    for m, kw, word in ((mol, dict(label_smoothing=M_EPS), "softmax head"), (model, dict(label_smoothing=M_EPS, teacher_logits=tl), "teacher_logits"),
                        (model, dict(label_smoothing=1.0), "label_smoothing"), (model, dict(normalize="sum"), "normalize"),
                        (model, dict(class_weights=-wd.cpu()), "class_weights"), (model, dict(position_weights=rd[:, :-1]), "position_weights")):
        def bad():
            try:
                m.loss_and_backward(xd, hd, td, micro_step=(0, 2), **kw)
            except ValueError as e:
                assert word in str(e), (kw, str(e))
            else:
                raise AssertionError("loss_and_backward took %r" % (sorted(kw),))
        assert not PC.launch_log(lib, bad), sorted(kw)
    model.loss_and_backward(xd, hd, td)   # (a plain call inside a cycle would raise)
    # a host weight tensor is checked and uploaded once, not once per step
    host_w = wd.cpu()
    model.loss_and_backward(xd, hd, td, class_weights=host_w)
    first = eng._weights_seen["class_weights"]
    model.loss_and_backward(xd, hd, td, class_weights=host_w)
    assert eng._weights_seen["class_weights"] is first and first[0]() is host_w


def check_model_launches(lib, dev):
    model, xd, hd, td, wd, rd, ts = _model(lib, dev)
    eng = model.engine
    opts = dict(class_weights=wd, label_smoothing=M_EPS, position_weights=rd)
    seq = PC.launch_sequence(eng.lib, lambda: model.loss_and_backward(xd, hd, td, **opts))
    assert "softmax_ce" not in seq and "fwd_post2_ce" not in seq, seq
    i = seq.index("ce_divisor")
    assert seq[i:i + 4] == ["ce_divisor", "ce_divisor_tail", "softmax_cew", "cew_reduce"] and seq.count("softmax_cew") == 1, seq
    # the divisor is summed on the device only where it depends on the data
    for kw in (dict(label_smoothing=M_EPS), dict(class_weights=wd, normalize="positions")):
        seq_n = PC.launch_sequence(eng.lib, lambda: model.loss_and_backward(xd, hd, td, **kw))
        assert "ce_divisor" not in seq_n and seq_n.count("softmax_cew") == 1 and seq_n.count("cew_reduce") == 1, seq_n
    # the backward pass behind the weighted loss takes the measured maximum: the launch sequence behind engine.loss, no scan
    logits = eng.forward(xd, hd)
    _, dl_ce = eng.loss(logits, td, t_start=ts)
    seq_ce = PC.launch_sequence(eng.lib, lambda: eng.backward(dl_ce, t_first=ts))
    logits = eng.forward(xd, hd)
    _, dl = eng.weighted_loss(logits, td, t_start=ts, **opts)
    seq_b = PC.launch_sequence(eng.lib, lambda: eng.backward(dl, t_first=ts))
    assert seq_b == seq_ce, (seq_b, seq_ce)
    g_word = eng.grads().cpu().clone()
    seq_scan = PC.launch_sequence(eng.lib, lambda: eng.backward(dl.clone(), t_first=ts, dlogits_bound=None))
    assert len(seq_scan) > len(seq_b), "another tensor object must make the library scan for its maximum"
    g_scan = eng.grads().cpu().clone()
    cfg = model_instance()[0]
    gw, gsn = PC.flat_to_state(eng, g_word, O.param_shapes(cfg)), PC.flat_to_state(eng, g_scan, O.param_shapes(cfg))
    for k in gw:
        e = PC.rel_to_max(gw[k], gsn[k])
        assert e <= PC.TOL_GRAD, (k, e)
    # identity: the keywords at their defaults -- spelled out or not, "positions" alone included -- are the fused step, launch
    # for launch, bit for bit
    box = {}
    seq0 = PC.launch_sequence(eng.lib, lambda: box.update(loss=model.loss_and_backward(xd, hd, td)))
    loss0, g0 = _b(box["loss"]), _b(eng.grads())
    assert "fwd_post2_ce" in seq0 and "softmax_cew" not in seq0
    for kw in (dict(class_weights=None, label_smoothing=0.0, position_weights=None, normalize="weights"), dict(normalize="positions")):
        eng.grads().fill_(float("nan"))
        box = {}
        assert PC.launch_sequence(eng.lib, lambda: box.update(loss=model.loss_and_backward(xd, hd, td, **kw))) == seq0, kw
        assert torch.equal(_b(box["loss"]), loss0) and torch.equal(_b(eng.grads()), g0), kw


def check_model_frozen(lib, dev):
    model, xd, hd, td, wd, rd, ts = _model(lib, dev)
    eng = model.engine
    frozen = FC.apply_freeze(model, "bottom:1", eng.n_layers)
    assert frozen
    ts_set = model.trainable()
    opts = dict(class_weights=wd, label_smoothing=M_EPS, position_weights=rd)
    _, g = _by_hand(model, xd, hd, td, opts, ts, first_layer=ts_set.first_layer, needs=ts_set.needs)
    model.loss_and_backward(xd, hd, td, **opts)
    flat = g.view(torch.float32)
    for (k, p), (off, n, shape, dead) in zip(model.named_parameters(), model._param_slices):
        if k in frozen or dead:
            assert p.grad is None, k
        else:
            assert torch.equal(_b(p.grad), _b(flat[off:off + n].view(shape))), k


def check_model_numerics(lib, dev):
    """Every parameter gradient against fp64 autograd of torch's criterion through the oracle's network, with the HIP path's own
    ReLU sub-gradient choice (check_model_numerics of tests/distill_common.py)."""
    cfg, params, x, h, t, w, r = model_instance()
    model, xd, hd, td, wd, rd, ts = _model(lib, dev)
    eng = model.engine
    for lengths in (None, list(M_LENGTHS)):
        loss = model.loss_and_backward(xd, hd, td, class_weights=wd, label_smoothing=M_EPS, lengths=lengths)
        grads = PC.flat_to_state(eng, eng.grads().cpu(), O.param_shapes(cfg))
        m_skip = (eng.saved(_lib.WS_RELU_SKIP) > 0).double().cpu()
        m_post = (eng.saved(_lib.WS_RELU_POST1) > 0).double().cpu()
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
        out = O.forward(cfg, leaves, x, h.double(), relu_masks=(m_skip, m_post))     # (B, T, Q)
        live = LC.live_mask(M_B, M_T, ts, lengths)
        l = F.cross_entropy(out[live], t[live], weight=w.double(), label_smoothing=M_EPS)
        l.backward()
        assert abs(float(loss.cpu()) - float(l.detach())) <= PC.TOL_LOSS, (float(loss.cpu()), float(l.detach()))
        for k, v in leaves.items():
            if v.grad is None or float(v.grad.abs().max()) == 0.0:
                assert float(grads[k].abs().max()) == 0.0, k
                continue
            e = PC.rel_to_max(grads[k], v.grad.float())
            assert e <= PC.TOL_GRAD, (k, e, lengths)
