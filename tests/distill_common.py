# -*- coding: utf-8 -*-
"""The soft-target (knowledge distillation) loss head: checks shared by tests/test_emu_distill.py (host emulator) and
tests/test_gpu_distill.py (MI355X).

Per live position, with s the student's and u the teacher's logit column, y the target, P = softmax(u / tau), S = softmax(s / tau):

    ce = logsumexp(s) - s_y,  kl = sum_q P_q (log P_q - log S_q),  l = (1 - alpha) ce + alpha tau^2 kl
    d_q = (1 - alpha) (softmax(s)_q - [q == y]) + alpha tau (S_q - P_q)          (dlogits / (grad_scale / N))

References: fp64, from the fp32 inputs the kernel sees.  Yardstick for what fp32 can do: the same formulas by torch on the CPU in
fp32 (``log_softmax((v - v.amax(1, keepdim=True)) / tau, 1)``) -- the convention of tests/loss_common.py, whose factor 4 and 8 u
terms these gates take over (u = 2^-24); none was fitted to the kernel:

    dlogits, per live position   max_q |d_k - d_64|  <=  4 E32 + 8 u ((1 - alpha) + 2 alpha tau)
    pos_loss, per live position  |l_k - l_64|        <=  4 e32 + 8 u max(1, |l_64|)
    loss[0..2]                   the sum of the per-position bounds + 2^-22 sum |.|, over N   (check_mean's form)

With alpha == 1 the kernel reads no target and reports ce = 0 (loss[1] == 0); with alpha == 0, l = ce."""
import ctypes
import functools
import math

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle, load_state_into_flat
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import freeze_common as FC
from tests import loss_common as LC
from tests import parity_common as PC

U24 = LC.U24
FACTOR = LC.FACTOR
OP_B, OP_T, OP_T_START, OP_GRAD_SCALE = LC.OP_B, LC.OP_T, LC.OP_T_START, LC.OP_GRAD_SCALE
OP_LENGTHS = LC.OP_LENGTHS
OP_Q = (37, 64, 256, 300)          # a ragged quarter per wave, the plain case, the full register-resident case, the two-pass route
OP_AT = ((0.3, 2.0), (1.0, 1.0), (0.7, 0.5))
OP_MODES = ("dense", "ragged", "full")
# the emulator's subset: every Q, every (alpha, tau), dense and ragged
EMU_MATRIX = [(37, 0.3, 2.0, ("dense", "full")), (64, 1.0, 1.0, ("ragged",)), (256, 0.7, 0.5, ("dense",)), (300, 0.3, 2.0, ("ragged",)),
              (256, 1.0, 1.0, ("ragged",))]
PATTERNS = [p for p in LC.PATTERNS if p[0] != "P4"]
assert OP_T - 256 >= len(PATTERNS)   # every pattern also lands in the ragged last block


def _log_softmax_t(v, tau):
    return torch.log_softmax((v - v.amax(1, keepdim=True)) / tau, 1)


def _formulas(s, u, hot, tq, alpha, tau):
    """The definition in the dtype of s / u: per position ce, kl, l (B, T) and per class d (B, Q, T)."""
    ls1 = _log_softmax_t(s, 1.0)
    lsS = ls1 if tau == 1.0 else _log_softmax_t(s, tau)
    lsP = _log_softmax_t(u, tau)
    P, S, p1 = torch.exp(lsP), torch.exp(lsS), torch.exp(ls1)
    ce = -ls1.gather(1, tq[:, None, :])[:, 0]
    kl = torch.where(P > 0, P * (lsP - lsS), torch.zeros_like(P)).sum(1)
    if alpha == 1.0:
        ce = torch.zeros_like(ce)
        l = tau * tau * kl
    elif alpha == 0.0:
        l = ce
    else:
        l = (1.0 - alpha) * ce + alpha * tau * tau * kl
    d = (1.0 - alpha) * (p1 - hot.to(s.dtype)) + alpha * tau * (S - P)
    return ce, kl, l, d


def distill_refs(s32, u32, target, alpha, tau):
    B, Q, T = s32.shape
    tq = torch.remainder(target, Q)
    hot = torch.zeros((B, Q, T), dtype=torch.bool).scatter_(1, tq[:, None, :], True)
    ce, kl, l, d = _formulas(s32.double(), u32.double(), hot, tq, alpha, tau)
    ce32, kl32, l32, d32 = _formulas(s32, u32, hot, tq, alpha, tau)
    r = dict(tq=tq, hot=hot, ce=ce, kl=kl, l=l, d=d)
    r["E_d"] = (d32.double() - d).abs().amax(1)
    for k, a32, a in (("ce", ce32, ce), ("kl", kl32, kl), ("l", l32, l)):
        r["e_" + k] = torch.where(torch.isfinite(a), (a32.double() - a).abs(), torch.zeros_like(a))
    return r


def pos_bound(ref, what):
    v = ref[what]
    b = FACTOR * ref["e_" + what] + 8 * U24 * v.abs().clamp(min=1.0)
    return torch.where(torch.isfinite(v), b, torch.full_like(b, float("inf")))


def check_grad(tag, dk, ref, live, unit, alpha, tau, fam):
    dk = dk.cpu()
    dead = ~live[:, None, :].expand_as(dk)
    if bool(dead.any()):
        assert float(dk[dead].abs().max()) == 0.0, tag
    err = (dk.double() / unit - ref["d"]).abs().amax(1)
    gate = FACTOR * ref["E_d"] + 8 * U24 * ((1.0 - alpha) + 2.0 * alpha * tau)
    frac = torch.where(live, err / gate, torch.zeros_like(err))
    b, t = divmod(int(frac.argmax()), frac.shape[1])
    print("FIGURE %s dlogits: worst of-gate %.3g at b=%d t=%d %s (err %.3g, torch fp32 %.3g)"
          % (tag, float(frac[b, t]), b, t, fam[t], float(err[b, t]), float(ref["E_d"][b, t])))
    bad = ["%s b=%d t=%d %s: |d_k - d_64| = %.3g > %.3g" % (tag, b, t, fam[t], float(err[b, t]), float(gate[b, t]))
           for b in range(err.shape[0]) for t in range(err.shape[1]) if bool(live[b, t]) and not float(err[b, t]) <= float(gate[b, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])


def check_pos(tag, pos, ref, live, fam):
    pos = pos.cpu().double()
    if bool((~live).any()):
        assert float(pos[~live].abs().max()) == 0.0, tag
    err, gate = (pos - ref["l"]).abs(), pos_bound(ref, "l")
    frac = torch.where(live, err / gate, torch.zeros_like(err))
    b, t = divmod(int(frac.argmax()), frac.shape[1])
    print("FIGURE %s pos_loss: worst of-gate %.3g at b=%d t=%d %s (err %.3g, torch fp32 %.3g)"
          % (tag, float(frac[b, t]), b, t, fam[t], float(err[b, t]), float(ref["e_l"][b, t])))
    bad = ["%s b=%d t=%d %s: |l_k - l_64| = %.3g > %.3g (l_64 = %.9g)" % (tag, b, t, fam[t], float(err[b, t]), float(gate[b, t]), float(ref["l"][b, t]))
           for b in range(err.shape[0]) for t in range(err.shape[1]) if bool(live[b, t]) and not float(err[b, t]) <= float(gate[b, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])


def mean_bound(ref, what, live):
    n = int(live.sum())
    return (float(pos_bound(ref, what)[live].sum()) + 2.0 ** -22 * float(ref[what][live].abs().sum())) / n


def check_means(tag, loss3, ref, live):
    n = int(live.sum())
    got = [float(v) for v in loss3.cpu()]
    for i, what in enumerate(("l", "ce", "kl")):
        want = float(ref[what][live].sum()) / n
        bound = mean_bound(ref, what, live)
        print("FIGURE %s loss[%d] (%s): %.9g, fp64 %.9g, err %.3g (bound %.3g)" % (tag, i, what, got[i], want, abs(got[i] - want), bound))
        assert abs(got[i] - want) <= bound, (tag, what, got[i], want, abs(got[i] - want), bound)


@functools.lru_cache(maxsize=None)
def op_inputs(Q):
    """(student (B, Q, T), teacher (B, Q, T), target (B, T), family per t): position t carries pattern t % len(PATTERNS) in the
    student and, drawn with another seed and another peak class, in the teacher -- peaks and offsets of the two disagree."""
    B, T = OP_B, OP_T
    out = []
    tg = np.zeros((B, T), dtype=np.int64)
    for which, seed in (("student", 6000 + Q), ("teacher", 7000 + Q)):
        rs = np.random.RandomState(seed)
        v = np.zeros((B, Q, T), dtype=np.float32)
        for t in range(T):
            shift = 0 if which == "student" else 5
            _, gen = PATTERNS[(t + shift) % len(PATTERNS)]
            for b in range(B):
                col, tq = gen(rs, Q, int(rs.randint(Q)))
                v[b, :, t] = col.astype(np.float32)
                if which == "student":
                    tg[b, t] = tq + Q * int(rs.randint(-2, 3))       # modulo Q
        out.append(torch.from_numpy(v))
    fam = [PATTERNS[t % len(PATTERNS)][0] for t in range(T)]
    return out[0], out[1], torch.from_numpy(tg), fam


@functools.lru_cache(maxsize=None)
def op_refs(Q, alpha, tau):
    s, u, t, _ = op_inputs(Q)
    return distill_refs(s, u, t, alpha, tau)


def op_engine(Q, lib, device):
    return WaveNetEngine(Q, *LC.OP_CFG_TAIL, device=device, library=lib)


def _b(t):
    return t.detach().cpu().clone().contiguous().view(torch.int32)


def check_distill_op(Q, alpha, tau, modes, lib, device):
    s32, u32, target, fam = op_inputs(Q)
    ref = op_refs(Q, alpha, tau)
    B, T, ts, gs = OP_B, OP_T, OP_T_START, OP_GRAD_SCALE
    eng = op_engine(Q, lib, device)
    sd, ud, td = s32.to(device), u32.to(device), target.to(device)
    dense = None
    for name in modes:
        lengths = {"dense": None, "ragged": list(OP_LENGTHS), "full": [T] * B}[name]
        live = LC.live_mask(B, T, ts, lengths)
        n = int(live.sum())
        tag = "distill Q=%d a=%g tau=%g %s" % (Q, alpha, tau, name)
        loss3, dl, pos = eng.distill_loss(sd, ud, td, alpha, tau, ts, gs, lengths=lengths, want_pos=True)
        # bit-level invariants: without the gradient and the per-position loss; a second call; NaN in scratch and workspace
        l0, none = eng.distill_loss(sd, ud, td, alpha, tau, ts, gs, lengths=lengths, want_grad=False)
        assert none is None and torch.equal(_b(l0), _b(loss3)), tag
        eng._distill_scratch.fill_(float("nan"))
        eng.workspace(B, T).fill_(float("nan"))
        l1, dl1, pos1 = eng.distill_loss(sd, ud, td, alpha, tau, ts, gs, lengths=lengths, want_pos=True)
        eng._distill_scratch.zero_()
        eng.workspace(B, T).zero_()
        l2, dl2, pos2 = eng.distill_loss(sd, ud, td, alpha, tau, ts, gs, lengths=lengths, want_pos=True)
        for a, b, c in ((loss3, l1, l2), (dl, dl1, dl2), (pos, pos1, pos2)):
            assert torch.equal(_b(a), _b(b)) and torch.equal(_b(a), _b(c)), tag
        if name == "dense":
            dense = (_b(loss3), _b(dl), _b(pos))
        if name == "full":
            if dense is None:
                d3, dd, dp = eng.distill_loss(sd, ud, td, alpha, tau, ts, gs, want_pos=True)
                dense = (_b(d3), _b(dd), _b(dp))
            assert torch.equal(_b(loss3), dense[0]) and torch.equal(_b(dl), dense[1]) and torch.equal(_b(pos), dense[2]), tag
            continue
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pos).all()), tag
        check_grad(tag, dl, ref, live, gs / n, alpha, tau, fam)
        check_pos(tag, pos, ref, live, fam)
        check_means(tag, loss3, ref, live)
        if alpha == 1.0:   # the target is not read: garbage changes no bit, and neither does its absence
            junk = torch.full_like(target, 0x7edcba9876543210).to(device)
            for tj in (junk, None):
                lj, dj, pj = eng.distill_loss(sd, ud, tj, alpha, tau, ts, gs, lengths=lengths, want_pos=True)
                assert torch.equal(_b(lj), _b(loss3)) and torch.equal(_b(dj), _b(dl)) and torch.equal(_b(pj), _b(pos)), tag
            assert float(loss3[1].cpu()) == 0.0
        # the teacher equal to the student's own logits: no divergence, and the total is the weighted cross-entropy
        ls, _ = eng.distill_loss(sd, sd, td, alpha, tau, ts, gs, lengths=lengths)
        ls = [float(v) for v in ls.cpu()]
        assert abs(ls[2]) <= 8 * U24, (tag, ls)
        rs = distill_refs(s32, s32, target, alpha, tau)
        assert abs(ls[0] - (1.0 - alpha) * ls[1]) <= mean_bound(rs, "l", live), (tag, ls)


SMALL_T = LC.SMALL_T
MASK_Q = (37, 256)
MASKED = (1, 9, 20)


def _small(Q, seed):
    rs = np.random.RandomState(seed)
    s = torch.from_numpy(rs.standard_normal((1, Q, SMALL_T)).astype(np.float32))
    u = torch.from_numpy(rs.standard_normal((1, Q, SMALL_T)).astype(np.float32))
    t = torch.from_numpy(rs.randint(0, Q, size=(1, SMALL_T)).astype(np.int64))
    for q in MASKED:   # the targets stay off the classes the cases mask
        t[t == q] = q + 1
    return s, u, t


def check_distill_masked(Q, lib, device):
    eng = op_engine(Q, lib, device)
    s, u, t = _small(Q, 6100 + Q)
    alpha, tau = 0.3, 2.0
    live = LC.live_mask(1, SMALL_T, 0)
    fam = ["M"] * SMALL_T
    for fill in (-float("inf"), -1e30):
        # the teacher masks classes the student keeps: finite everywhere, and those classes add exactly 0 to kl
        um = u.clone()
        um[0, list(MASKED), :] = fill
        ref = distill_refs(s, um, t, alpha, tau)
        loss3, dl, pos = eng.distill_loss(s.to(device), um.to(device), t.to(device), alpha, tau, 0, 1.0, want_pos=True)
        assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(pos).all()), fill
        tag = "distill Q=%d teacher masked %g" % (Q, fill)
        check_grad(tag, dl, ref, live, 1.0 / SMALL_T, alpha, tau, fam)
        check_pos(tag, pos, ref, live, fam)
        check_means(tag, loss3, ref, live)
        # both mask the same classes: dlogits there is exactly 0
        sm = s.clone()
        sm[0, list(MASKED), :] = fill
        loss3, dl = eng.distill_loss(sm.to(device), um.to(device), t.to(device), alpha, tau, 0, 1.0)
        assert bool(torch.isfinite(loss3).all()) and bool(torch.isfinite(dl).all()), fill
        assert float(dl.cpu()[0, list(MASKED), :].abs().max()) == 0.0, fill
        check_grad(tag + " both", dl, distill_refs(sm, um, t, alpha, tau), live, 1.0 / SMALL_T, alpha, tau, fam)
    # the student masks a class where the teacher has mass: +inf as torch gives, dlogits finite
    sm = s.clone()
    sm[0, MASKED[0], 3] = -float("inf")
    ref32 = _formulas(sm, u, torch.zeros((1, Q, SMALL_T), dtype=torch.bool).scatter_(1, t[:, None, :], True), t, alpha, tau)
    assert float(ref32[1].sum()) == float("inf") and float(ref32[2].sum()) == float("inf")
    loss3, dl, pos = eng.distill_loss(sm.to(device), u.to(device), t.to(device), alpha, tau, 0, 1.0, want_pos=True)
    l = [float(v) for v in loss3.cpu()]
    assert l[0] == float("inf") and l[2] == float("inf") and math.isfinite(l[1]), l
    assert bool(torch.isfinite(dl).all())
    assert float(pos.cpu()[0, 3]) == float("inf") and bool(torch.isfinite(pos.cpu()[0, [c for c in range(SMALL_T) if c != 3]]).all())
    check_grad("distill Q=%d student masked" % Q, dl, distill_refs(sm, u, t, alpha, tau), live, 1.0 / SMALL_T, alpha, tau, fam)


def check_distill_nonfinite(Q, lib, device):
    """One NaN, and in another call one +inf, in one student column, then in one teacher column: the loss and that column's
    ``dlogits`` are non-finite, every other column has the bits of the clean call."""
    eng = op_engine(Q, lib, device)
    s, u, t = _small(Q, 6200 + Q)
    col = 3
    keep = [c for c in range(SMALL_T) if c != col]
    for alpha, tau in ((0.3, 2.0), (0.7, 1.0)):
        _, base = eng.distill_loss(s.to(device), u.to(device), t.to(device), alpha, tau, 0, 1.0)
        base = base.cpu().clone()
        for who in ("student", "teacher"):
            for bad in (float("nan"), float("inf")):
                sb, ub = s.clone(), u.clone()
                (sb if who == "student" else ub)[0, (int(t[0, col]) + 1) % Q, col] = bad
                loss3, dl = eng.distill_loss(sb.to(device), ub.to(device), t.to(device), alpha, tau, 0, 1.0)
                dl = dl.cpu()
                assert not math.isfinite(float(loss3[0].cpu())), (who, bad)
                assert not bool(torch.isfinite(dl[0, :, col]).any()), (who, bad, dl[0, :, col])
                assert torch.equal(_b(dl[:, :, keep]), _b(base[:, :, keep])), (who, bad)


def check_distill_errors(lib, device):
    Q, B, T = 37, 1, SMALL_T
    eng = op_engine(Q, lib, device)
    s, u, t = (a.to(device) for a in _small(Q, 6300))
    ws = eng.workspace(B, T)
    loss = torch.zeros(3, dtype=torch.float32, device=device)
    scratch = torch.zeros(int(eng.lib.wn_softmax_distill_scratch_floats(B, T)), dtype=torch.float32, device=device)
    assert scratch.numel() >= 3
    assert eng.lib.wn_softmax_distill_scratch_floats(2, 304) >= 3 * 2 * 5

    def call(cfg=None, logits=s, teacher=u, target=t, t_start=0, n_loss=B * T, alpha=0.5, tau=1.0, out=loss, scr=scratch):
        return eng.lib.wn_softmax_distill_loss(ctypes.byref(cfg or eng.cfg), B, T, _ptr(logits), _ptr(teacher), _ptr(target), t_start,
                                               None, n_loss, alpha, tau, 1.0, 1.0, _ptr(out), None, None, _ptr(scr), _ptr(ws),
                                               ws.numel() * 4, _stream_handle(eng.device))

    assert call() == 0, eng.lib.wn_last_error().decode()
    assert call(target=None, alpha=1.0) == 0, eng.lib.wn_last_error().decode()
    for kw, word in ((dict(alpha=-0.1), "alpha"), (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"),
                     (dict(tau=0.0), "tau"), (dict(tau=-1.0), "tau"), (dict(tau=float("inf")), "tau"), (dict(tau=float("nan")), "tau"),
                     (dict(logits=None), "logits"), (dict(teacher=None), "teacher_logits"), (dict(target=None), "target"),
                     (dict(out=None), "loss"), (dict(scr=None), "scratch"), (dict(n_loss=0), "n_loss"), (dict(n_loss=B * T - 1), "n_loss"),
                     (dict(t_start=T), "t_start")):
        loss.fill_(7.0)
        assert call(**kw) != 0, kw
        msg = eng.lib.wn_last_error().decode()
        assert word in msg, (kw, msg)
        if "out" not in kw:
            assert float(loss.cpu()[0]) == 7.0, kw   # an error code, never a launch
    mol = WaveNetEngine(Q, *LC.OP_CFG_TAIL, device=device, library=lib, out_channels=3 * 4)
    wsm = mol.workspace(B, T)
    rc = mol.lib.wn_softmax_distill_loss(ctypes.byref(mol.cfg), B, T, _ptr(s), _ptr(u), _ptr(t), 0, None, B * T, 0.5, 1.0, 1.0, 1.0,
                                         _ptr(loss), None, None, _ptr(scratch), _ptr(wsm), wsm.numel() * 4, _stream_handle(mol.device))
    assert rc != 0 and "out_channels" in mol.lib.wn_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# model level: WaveNet.loss_and_backward(teacher_logits=...)
# ---------------------------------------------------------------------------------------------------------------------
STUDENT = (128, 4, 64, 128, 2, 1, 2, 0)
TEACHER = (128, 4, 64, 128, 3, 1, 2, 0)
M_B, M_T = 2, 272
M_LENGTHS = (150, M_T)
M_ALPHA, M_TAU = 0.6, 2.0


@functools.lru_cache(maxsize=None)
def model_instance():
    cfg, tcfg = O.OracleConfig(*STUDENT), O.OracleConfig(*TEACHER)
    params, x, h, t, _, _ = PC.pick_instance(cfg, M_B, M_T, 8100, 0.3)
    tparams = O.random_params(tcfg, 8200, scale=0.3)
    return cfg, tcfg, params, tparams, x, h, t


def _models(lib, dev):
    cfg, tcfg, params, tparams, x, h, t = model_instance()
    student, teacher = WaveNet(*STUDENT, _library=lib), WaveNet(*TEACHER, _library=lib)
    student.load_state_dict(params)
    teacher.load_state_dict(tparams)
    student.to(dev)
    teacher.to(dev)
    teacher.requires_grad_(False)
    xd, hd, td = x.to(dev), h.to(dev), t.to(dev)
    tl = teacher.teacher_logits(xd, hd)
    assert tuple(tl.shape) == (M_B, STUDENT[0], M_T) and not tl.requires_grad
    t_start = max(cfg.receptive_field, tcfg.receptive_field)
    assert t_start == tcfg.receptive_field > cfg.receptive_field
    return student, tl, xd, hd, td, t_start


def _by_hand(student, tl, xd, hd, td, t_start, grad_scale=1.0, lengths=None, dh=None, **needs):
    eng = student.engine
    logits = eng.forward(xd, hd)
    loss3, dl = eng.distill_loss(logits, tl, td, M_ALPHA, M_TAU, t_start=t_start, grad_scale=grad_scale, lengths=lengths)
    flat = eng.backward(dl, t_first=t_start, dh=dh, **needs)
    return _b(loss3), _b(flat)


def check_model_composition(lib, dev):
    student, tl, xd, hd, td, ts = _models(lib, dev)
    eng = student.engine
    kw = dict(teacher_logits=tl, distill_alpha=M_ALPHA, distill_temperature=M_TAU, t_start=ts)
    for lengths in (None, list(M_LENGTHS)):
        l3, g = _by_hand(student, tl, xd, hd, td, ts, lengths=lengths)
        eng.grads().fill_(float("nan"))
        loss = student.loss_and_backward(xd, hd, td, lengths=lengths, **kw)
        assert tuple(loss.shape) == (1,) and torch.equal(_b(loss), l3[0:1]) and torch.equal(_b(student.distill_parts), l3)
        assert torch.equal(_b(eng.grads()), g), lengths
        # aux_grad: the same dh
        dh0 = torch.empty_like(hd)
        _, g2 = _by_hand(student, tl, xd, hd, td, ts, lengths=lengths, dh=dh0)
        loss, dh = student.loss_and_backward(xd, hd, td, lengths=lengths, aux_grad=True, **kw)
        assert torch.equal(_b(dh), _b(dh0)) and torch.equal(_b(eng.grads()), g2) and torch.equal(_b(loss), l3[0:1])
    # two micro-steps: the sum of the hand-composed halves
    _, ga = _by_hand(student, tl, xd, hd, td, ts, grad_scale=0.5)
    _, gb = _by_hand(student, tl, xd, hd, td, ts, grad_scale=0.5, lengths=list(M_LENGTHS))
    student.loss_and_backward(xd, hd, td, grad_scale=0.5, micro_step=(0, 2), **kw)
    student.loss_and_backward(xd, hd, td, grad_scale=0.5, lengths=list(M_LENGTHS), micro_step=(1, 2), **kw)
    assert torch.equal(_b(eng.grads()), _b(ga.view(torch.float32) + gb.view(torch.float32)))
    # a mixture head raises
    mol = WaveNet(*STUDENT, n_mixture=2, _library=lib).to(dev)
    try:
        mol.loss_and_backward(xd, hd, td, teacher_logits=tl)
    except ValueError as e:
        assert "softmax head" in str(e)
    else:
        raise AssertionError("a mixture-head model took teacher_logits")


def check_model_launches(lib, dev):
    student, tl, xd, hd, td, ts = _models(lib, dev)
    eng = student.engine
    kw = dict(teacher_logits=tl, distill_alpha=M_ALPHA, distill_temperature=M_TAU, t_start=ts)
    log = PC.launch_log(eng.lib, lambda: student.loss_and_backward(xd, hd, td, **kw))
    assert log.get("softmax_distill") == 1 and "softmax_ce" not in log and "fwd_post2_ce" not in log, log
    # the backward pass behind the distill loss takes the measured maximum: the launch sequence behind engine.loss, no scan
    logits = eng.forward(xd, hd)
    _, dl_ce = eng.loss(logits, td, t_start=ts)
    seq_ce = PC.launch_sequence(eng.lib, lambda: eng.backward(dl_ce, t_first=ts))
    logits = eng.forward(xd, hd)
    _, dl = eng.distill_loss(logits, tl, td, M_ALPHA, M_TAU, t_start=ts)
    seq = PC.launch_sequence(eng.lib, lambda: eng.backward(dl, t_first=ts))
    assert seq == seq_ce, (seq, seq_ce)
    g_word = eng.grads().cpu().clone()
    seq_scan = PC.launch_sequence(eng.lib, lambda: eng.backward(dl.clone(), t_first=ts, dlogits_bound=None))
    assert len(seq_scan) > len(seq), "another tensor object must make the library scan for its maximum"
    g_scan = eng.grads().cpu().clone()
    cfg = model_instance()[0]
    gw, gsn = PC.flat_to_state(eng, g_word, O.param_shapes(cfg)), PC.flat_to_state(eng, g_scan, O.param_shapes(cfg))
    for k in gw:
        e = PC.rel_to_max(gw[k], gsn[k])
        assert e <= PC.TOL_GRAD, (k, e)
    # identity: no teacher, and a teacher with alpha == 0, are the plain call -- launch for launch, bit for bit
    seq0 = PC.launch_sequence(eng.lib, lambda: student.loss_and_backward(xd, hd, td, t_start=ts))
    loss0, g0 = _b(student.loss_and_backward(xd, hd, td, t_start=ts)), _b(eng.grads())
    seq1 = PC.launch_sequence(eng.lib, lambda: student.loss_and_backward(xd, hd, td, t_start=ts, teacher_logits=None))
    seq2 = PC.launch_sequence(eng.lib, lambda: student.loss_and_backward(xd, hd, td, t_start=ts, teacher_logits=tl, distill_alpha=0.0))
    assert seq1 == seq0 and seq2 == seq0 and "softmax_distill" not in seq0
    loss2 = student.loss_and_backward(xd, hd, td, t_start=ts, teacher_logits=tl, distill_alpha=0.0)
    assert torch.equal(_b(loss2), loss0) and torch.equal(_b(eng.grads()), g0)


def check_model_frozen(lib, dev):
    student, tl, xd, hd, td, ts = _models(lib, dev)
    eng = student.engine
    frozen = FC.apply_freeze(student, "bottom:1", eng.n_layers)
    assert frozen
    ts_set = student.trainable()
    _, g = _by_hand(student, tl, xd, hd, td, ts, first_layer=ts_set.first_layer, needs=ts_set.needs)
    student.loss_and_backward(xd, hd, td, teacher_logits=tl, distill_alpha=M_ALPHA, distill_temperature=M_TAU, t_start=ts)
    flat = g.view(torch.float32)
    for (k, p), (off, n, shape, dead) in zip(student.named_parameters(), student._param_slices):
        if k in frozen or dead:
            assert p.grad is None, k
        else:
            assert torch.equal(_b(p.grad), _b(flat[off:off + n].view(shape))), k


def check_model_numerics(lib, dev):
    """Every parameter gradient against fp64 autograd of the definition through the oracle's network, the teacher's logits taken
    from the HIP forward; the HIP path's own ReLU sub-gradient choice (run_mol_vs_restatement's method)."""
    cfg, tcfg, params, tparams, x, h, t = model_instance()
    student, tl, xd, hd, td, ts = _models(lib, dev)
    eng = student.engine
    for lengths in (None, list(M_LENGTHS)):
        loss = student.loss_and_backward(xd, hd, td, teacher_logits=tl, distill_alpha=M_ALPHA, distill_temperature=M_TAU, t_start=ts,
                                         lengths=lengths)
        grads = PC.flat_to_state(eng, eng.grads().cpu(), O.param_shapes(cfg))
        m_skip = (eng.saved(_lib.WS_RELU_SKIP) > 0).double().cpu()
        m_post = (eng.saved(_lib.WS_RELU_POST1) > 0).double().cpu()
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
        out = O.forward(cfg, leaves, x, h.double(), relu_masks=(m_skip, m_post)).transpose(1, 2)     # (B, Q, T)
        live = LC.live_mask(M_B, M_T, ts, lengths)
        u = tl.cpu().double()
        lsS, lsP = _log_softmax_t(out, M_TAU), _log_softmax_t(u, M_TAU)
        ce = -torch.log_softmax(out, 1).gather(1, t[:, None, :])[:, 0]
        kl = (torch.exp(lsP) * (lsP - lsS)).sum(1)
        l = ((1.0 - M_ALPHA) * ce + M_ALPHA * M_TAU ** 2 * kl)[live].sum() / int(live.sum())
        l.backward()
        assert abs(float(loss.cpu()) - float(l.detach())) <= PC.TOL_LOSS, (float(loss.cpu()), float(l.detach()))
        for k, v in leaves.items():
            if v.grad is None or float(v.grad.abs().max()) == 0.0:
                assert float(grads[k].abs().max()) == 0.0, k
                continue
            e = PC.rel_to_max(grads[k], v.grad.float())
            assert e <= PC.TOL_GRAD, (k, e, lengths)
