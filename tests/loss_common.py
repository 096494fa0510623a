# -*- coding: utf-8 -*-
"""The loss heads per position at the logits of a TRAINED model, against fp64: checks shared by tests/test_emu_loss.py (host
emulator) and tests/test_gpu_loss.py (MI355X).

Every other test feeds the heads the logits of a randomly initialised network (p ~ 1/Q everywhere) and divides a gradient
error by the largest element of the whole tensor.  Here every position is judged on its own, on the probability scale
``dlogits / (grad_scale / N)``, at distributions peaked by 20 - 110 nats, a common offset on the logits, masked classes, ties,
targets whose probability underflows -- and, for the fused epilogue, the row maximum in every lane half and wave row.

References: fp64, from the fp32 inputs the kernel sees.  Yardstick for what fp32 can do: the same formulas by torch on the CPU
in fp32 (``log_softmax`` / ``exp``; ``O.mol_nll`` in fp32).  With u = 2^-24 the gates are

  softmax, per live position      max_q |d_k - d_64| / (gs / N)  <=  4 E32 + 8 u
  every class with p_64 >= 1e-30  |p_k / p_64 - 1|               <=  4 (yardstick's) + 8 u (4 + |v_q - lse_64|)
  per-position loss               |nll_k - nll_64|               <=  4 (yardstick's) + 8 u max(1, |nll_64|)
  scalar loss, row sums           the sum of the per-position bounds + 2^-22 sum |nll_64|  (/ N for the mean)
  mixture head, per element       |d_k - d_64| / (gs / N)        <=  4 E32_elem + 16 u S (1 + max_i A_i)

(S = 1 for a mixture logit, inv_i = exp(-ls_i) for a mean, 1 + A_i for a log-scale, A_i = inv_i (|y - mean_i| + half_bin)).
The factor 4 is the room the hardware's 1-ulp v_exp_f32 / v_log_f32 / v_rcp_f32 and another summation order get over libm;
none of these numbers was fitted to a kernel.

The relative gate leaves out the TARGET class: the kernels return d_t = p_t - 1, from which p_t cannot be recovered once
p_t < u; the target element is held by the absolute gate, whose reference forms it as -sum_{q != t} p_q."""
import ctypes
import functools
import math

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, _ptr, _stream_handle, load_state_into_flat
from tests import mol_common as MC
from tests import parity_common as PC

U24 = 2.0 ** -24
P_FLOOR = 1e-30
FACTOR = 4.0

# ---------------------------------------------------------------------------------------------------------------------
# softmax head: references and gates
# ---------------------------------------------------------------------------------------------------------------------


def softmax_refs(v32, target):
    """v32 (B, Q, T) fp32, target (B, T) int64 (taken modulo Q like the kernels) -> dict of fp64 per-position references and
    the fp32 yardstick's errors against them.  d_64's target element is -sum_{q != t} p_q, so the reference does not cancel."""
    B, Q, T = v32.shape
    tq = torch.remainder(target, Q)
    hot = torch.zeros((B, Q, T), dtype=torch.bool).scatter_(1, tq[:, None, :], True)
    v = v32.double()
    lse = torch.logsumexp(v, dim=1)                                   # (B, T)
    p = torch.exp(v - lse[:, None, :])
    vt = v.gather(1, tq[:, None, :])[:, 0]
    nll = lse - vt
    others = torch.where(hot, torch.zeros_like(p), p).sum(dim=1)
    d = torch.where(hot, -others[:, None, :].expand_as(p), p)
    # the yardstick: torch fp32 on the same fp32 logits
    ls32 = torch.log_softmax(v32, dim=1)
    p32 = torch.exp(ls32)
    d32 = (p32 - hot.float()).double()
    nll32 = -ls32.gather(1, tq[:, None, :])[:, 0].double()
    finite = torch.isfinite(nll)
    e_d = (d32 - d).abs().amax(dim=1)                                  # (B, T)
    ok = (p >= P_FLOOR) & ~hot
    e_rel = torch.where(ok, (p32.double() / p.clamp(min=1e-300) - 1.0).abs(), torch.zeros_like(p))
    e_nll = torch.where(finite, (nll32 - nll).abs(), torch.zeros_like(nll))
    return dict(tq=tq, hot=hot, v=v, lse=lse, p=p, nll=nll, d=d, e_d=e_d, e_rel=e_rel, e_nll=e_nll, rel_ok=ok)


def nll_bound(ref):
    """Per-position bound on |nll_k - nll_64| (B, T); positions with a non-finite reference get +inf (checked by their own
    assertions)."""
    b = FACTOR * ref["e_nll"] + 8 * U24 * ref["nll"].abs().clamp(min=1.0)
    return torch.where(torch.isfinite(ref["nll"]), b, torch.full_like(b, float("inf")))


class Worst(object):
    """Running worst figures of one case family: the yardstick's error, the kernel's, and the kernel's as a fraction of its gate."""

    def __init__(self):
        self.rows = {}

    def note(self, family, what, kernel, yard, frac):
        k = (family, what)
        r = self.rows.get(k, (0.0, 0.0, 0.0))
        self.rows[k] = (max(r[0], kernel), max(r[1], yard), max(r[2], frac))

    def report(self, tag):
        for (family, what), (kernel, yard, frac) in sorted(self.rows.items()):
            print("FIGURE %s %-10s %-8s kernel %.3g  torch-fp32 %.3g  ratio %.3g  of-gate %.3g"
                  % (tag, family, what, kernel, yard, kernel / yard if yard > 0 else float("inf") if kernel > 0 else 0.0, frac))


def check_softmax_grad(tag, dk, ref, live, unit, family_of, worst=None, skip=None):
    """dk (B, Q, T) from the kernel, ``unit`` = grad_scale / N, ``live`` (B, T) bool, ``family_of`` (T,) list of family names.
    Exactly zero outside ``live``; the two per-position gates on it.  ``skip`` (B, T) bool: positions judged elsewhere."""
    dk = dk.cpu()
    B, Q, T = dk.shape
    dead = ~live[:, None, :].expand_as(dk)
    assert float(dk[dead].abs().max()) == 0.0 if bool(dead.any()) else True, tag
    judged = live if skip is None else live & ~skip
    dn = dk.double() / unit
    err = (dn - ref["d"]).abs().amax(dim=1)
    gate = FACTOR * ref["e_d"] + 8 * U24
    pk = dn                                                        # p of the non-target classes
    rel = torch.where(ref["rel_ok"], (pk / ref["p"].clamp(min=1e-300) - 1.0).abs(), torch.zeros_like(pk))
    rgate = FACTOR * ref["e_rel"] + 8 * U24 * (4.0 + (ref["v"] - ref["lse"][:, None, :]).abs())
    rgate = torch.where(ref["rel_ok"], rgate, torch.full_like(rgate, float("inf")))
    rfrac = (rel / rgate).amax(dim=1)
    bad = []
    for b in range(B):
        for t in range(T):
            if not bool(judged[b, t]):
                continue
            fam = family_of[t]
            if worst is not None:
                worst.note(fam, "d", float(err[b, t]), float(ref["e_d"][b, t]), float(err[b, t] / gate[b, t]))
                worst.note(fam, "p_rel", float(rel[b, :, t].max()), float(ref["e_rel"][b, :, t].max()), float(rfrac[b, t]))
            if not (float(err[b, t]) <= float(gate[b, t])):
                bad.append("%s b=%d t=%d %s: |d_k - d_64| = %.3g > %.3g (torch fp32: %.3g)"
                           % (tag, b, t, fam, float(err[b, t]), float(gate[b, t]), float(ref["e_d"][b, t])))
            if not (float(rfrac[b, t]) <= 1.0):
                q = int((rel[b, :, t] / rgate[b, :, t]).argmax())
                bad.append("%s b=%d t=%d %s: |p_k / p_64 - 1| = %.3g > %.3g at class %d (p_64 = %.3g, torch fp32: %.3g)"
                           % (tag, b, t, fam, float(rel[b, q, t]), float(rgate[b, q, t]), q, float(ref["p"][b, q, t]),
                              float(ref["e_rel"][b, q, t])))
    per_family = {f: sum(1 for m in bad if " %s: " % f in m) for f in sorted(set(family_of))}
    assert not bad, "\n".join(bad[:12] + ["... %d failures, per family %s" % (len(bad), per_family)])


def check_mean(tag, loss, ref, live, worst=None):
    """The scalar mean loss against the fp64 mean over ``live``: the sum of the per-position bounds plus 2^-22 sum |nll_64| for the
    fp32 block partials and the final rounding, over N."""
    n = int(live.sum())
    want = float(ref["nll"][live].sum()) / n
    bound = (float(nll_bound(ref)[live].sum()) + 2.0 ** -22 * float(ref["nll"][live].abs().sum())) / n
    got = float(loss.cpu())
    yard = float(ref["e_nll"][live].sum()) / n
    print("%s: mean loss %.9g, fp64 %.9g, err %.3g (bound %.3g)" % (tag, got, want, abs(got - want), bound))
    if worst is not None:
        worst.note("mean", "loss", abs(got - want), yard, abs(got - want) / bound)
    assert abs(got - want) <= bound, (tag, got, want, abs(got - want), bound)


def check_rows(tag, row, ref, live, worst=None):
    """Per-sequence sums against the per-position reference summed per sequence, same bound without the division."""
    row = row.cpu().double()
    for b in range(live.shape[0]):
        lv = live[b]
        if not bool(lv.any()):
            assert float(row[b]) == 0.0, (tag, b)
            continue
        want = float(ref["nll"][b][lv].sum())
        bound = float(nll_bound(ref)[b][lv].sum()) + 2.0 ** -22 * float(ref["nll"][b][lv].abs().sum())
        e = abs(float(row[b]) - want)
        print("%s row %d: %.9g, fp64 %.9g, err %.3g (bound %.3g)" % (tag, b, float(row[b]), want, e, bound))
        if worst is not None:
            worst.note("rows", "nll", e, float(ref["e_nll"][b][lv].sum()), e / bound)
        assert e <= bound, (tag, b, float(row[b]), want, e, bound)


def live_mask(B, T, t_start, lengths=None):
    m = torch.zeros((B, T), dtype=torch.bool)
    for b in range(B):
        m[b, t_start:(T if lengths is None else int(lengths[b]))] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 2. softmax head at op level: wn_softmax_ce_loss, wn_softmax_ce_loss_ragged, wn_softmax_nll_rows (k_softmax_ce)
# ---------------------------------------------------------------------------------------------------------------------
OP_B, OP_T, OP_T_START, OP_GRAD_SCALE = 2, 304, 5, 0.375
OP_LENGTHS = (100, OP_T)           # one sequence ends inside the first 256-thread block, the other at T
OP_Q = (37, 64, 300)               # a chunk-of-8 tail, the plain case, more than 256 classes
OP_CFG_TAIL = (4, 8, 12, 3, 2, 2, 4)


def _p0(rs, Q, t):
    return rs.standard_normal(Q), t


def _peaked_right(lift):
    def f(rs, Q, t):
        v = 3.0 * rs.standard_normal(Q)
        v[t] += lift
        return v, t
    return f


def _peaked_wrong(lift):
    def f(rs, Q, t):
        v = rs.standard_normal(Q)
        v[(t + 1 + rs.randint(Q - 1)) % Q] = v[t] + lift
        return v, t
    return f


def _offset(base, off):
    def f(rs, Q, t):
        v, t = base(rs, Q, t)
        return v + off, t
    return f


def _masked(rs, Q, t):
    v = rs.standard_normal(Q)
    others = [q for q in rs.permutation(Q) if q != t]
    for q in others[:3]:
        v[q] = -1e30
    for q in others[3:6]:
        v[q] = -np.inf
    return v, t


def _all_equal(rs, Q, t):
    return np.full(Q, 0.75), t


def _two_maxima(rs, Q, t):
    v = rs.standard_normal(Q)
    a = (t + 1 + rs.randint(Q - 1)) % Q
    v[a] = v[t] = 6.0
    return v, t


PATTERNS = [("P0", _p0)]
PATTERNS += [("P1", _peaked_right(l)) for l in (20.0, 60.0, 90.0)]
PATTERNS += [("P2", _peaked_wrong(l)) for l in (30.0, 95.0, 110.0)]
PATTERNS += [("P3", _offset(b, o)) for b in (_p0, _peaked_right(20.0)) for o in (1e3, -1e3, 3e4, -3e4)]
PATTERNS += [("P4", _masked), ("P5", _all_equal), ("P5", _two_maxima)]
assert OP_T - 256 >= len(PATTERNS)   # every pattern also lands in the ragged last block


@functools.lru_cache(maxsize=None)
def op_instance(Q):
    """(logits (B, Q, T) fp32, target (B, T) int64 -- some outside [0, Q): the kernels take them modulo Q --, family per t,
    references) of the one call that carries every pattern: position t has pattern t % len(PATTERNS)."""
    rs = np.random.RandomState(4000 + Q)
    B, T = OP_B, OP_T
    v = np.zeros((B, Q, T), dtype=np.float32)
    tg = np.zeros((B, T), dtype=np.int64)
    fam = []
    for t in range(T):
        name, gen = PATTERNS[t % len(PATTERNS)]
        fam.append(name)
        for b in range(B):
            col, tq = gen(rs, Q, int(rs.randint(Q)))
            v[b, :, t] = col.astype(np.float32)
            tg[b, t] = tq + Q * int(rs.randint(-2, 3))       # modulo Q
    v32, target = torch.from_numpy(v), torch.from_numpy(tg)
    return v32, target, fam, softmax_refs(v32, target)


def op_engine(Q, lib, device):
    return WaveNetEngine(Q, *OP_CFG_TAIL, device=device, library=lib)


def c_softmax_rows(eng, logits, td, t_start, t_end, acc=None):
    B, _, T = logits.shape
    ws = eng.eval_workspace(B, T)
    row = torch.full((B,), float("nan"), dtype=torch.float32, device=logits.device)
    rc = eng.lib.wn_softmax_nll_rows(ctypes.byref(eng.cfg), B, T, _ptr(logits), _ptr(td), int(t_start), _ptr(t_end), _ptr(row),
                                     _ptr(acc), _ptr(ws), ws.numel() * 4, _stream_handle(eng.device))
    assert rc == 0, eng.lib.wn_last_error().decode()
    return row


def check_softmax_op(Q, lib, device):
    """One dense and one ragged call over every pattern, judged per position; loss bits with and without a gradient; the
    ragged call with full lengths against the dense one; the rows with and without ``acc``; and each position's own loss."""
    v32, target, fam, ref = op_instance(Q)
    B, T, ts, gs = OP_B, OP_T, OP_T_START, OP_GRAD_SCALE
    eng = op_engine(Q, lib, device)
    vd, td = v32.to(device), target.to(device)
    worst = Worst()
    dense = None
    for name, lengths in (("dense", None), ("ragged", list(OP_LENGTHS)), ("full", [T] * B)):
        live = live_mask(B, T, ts, lengths)
        n = int(live.sum())
        loss, dl = eng.loss(vd, td, ts, gs, lengths=lengths)
        loss0, none = eng.loss(vd, td, ts, gs, lengths=lengths, want_grad=False)
        assert none is None and torch.equal(loss0.cpu(), loss.cpu()), (Q, name)
        if name == "dense":
            dense = (loss.cpu().clone(), dl.cpu().clone())
        if name == "full":
            assert torch.equal(loss.cpu(), dense[0]) and torch.equal(dl.cpu(), dense[1]), Q
            continue
        tag = "softmax_ce Q=%d %s" % (Q, name)
        check_softmax_grad(tag, dl, ref, live, gs / n, fam, worst)
        check_mean(tag, loss, ref, live, worst)
        # masked classes: exactly 0.0f
        masked = (v32 <= -1e30) & live[:, None, :]
        assert bool(masked.any()) and float(dl.cpu()[masked].abs().max()) == 0.0, tag
        # rows, with and without acc
        t_end = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(device)
        row = c_softmax_rows(eng, vd, td, ts, t_end)
        acc = torch.full((1,), 10.0, dtype=torch.float64, device=device)
        row_a = c_softmax_rows(eng, vd, td, ts, t_end, acc)
        assert torch.equal(row_a.cpu(), row.cpu())
        assert abs(float(acc.cpu()) - 10.0 - float(row.cpu().double().sum())) <= 1e-12 * float(row.cpu().double().sum())
        check_rows(tag, row, ref, live, worst)
    # every position's own loss: the rows of the same logits laid out as B * T sequences with one live position each (a sequence
    # is as long as the config's upsampling factor; t_end = 1 cuts it behind its first position)
    U = OP_CFG_TAIL[-1]
    v1 = torch.zeros((B * T, Q, U), dtype=torch.float32)
    v1[:, :, 0] = v32.permute(0, 2, 1).reshape(B * T, Q)
    t1 = torch.zeros((B * T, U), dtype=torch.int64)
    t1[:, 0] = target.reshape(B * T)
    ones = torch.ones(B * T, dtype=torch.int32).to(device)
    nll_k = c_softmax_rows(eng, v1.to(device), t1.to(device), 0, ones).cpu().double().reshape(B, T)
    err, bound = (nll_k - ref["nll"]).abs(), nll_bound(ref)
    for t in range(T):
        for b in range(B):
            worst.note(fam[t], "nll", float(err[b, t]), float(ref["e_nll"][b, t]), float(err[b, t] / bound[b, t]))
    bad = ["Q=%d b=%d t=%d %s: |nll_k - nll_64| = %.3g > %.3g (nll_64 = %.9g, torch fp32: %.3g)"
           % (Q, b, t, fam[t], float(err[b, t]), float(bound[b, t]), float(ref["nll"][b, t]), float(ref["e_nll"][b, t]))
           for b in range(B) for t in range(T) if not float(err[b, t]) <= float(bound[b, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])
    # P2 from 88 nats on: p_t underflows, the loss is still the finite lse - v_t and d_t = -grad_scale / N to rounding
    under = (ref["p"].gather(1, ref["tq"][:, None, :])[:, 0] < 1e-38)
    assert bool(under.any())
    assert bool(torch.isfinite(nll_k[under]).all()) and float((nll_k[under] - ref["nll"][under]).abs().max()) <= 8 * U24 * 128
    dt = dense[1].double().gather(1, ref["tq"][:, None, :])[:, 0] / (gs / (B * (T - ts)))
    assert float((dt[under & live_mask(B, T, ts)] + 1.0).abs().max()) <= 8 * U24
    worst.report("softmax_ce Q=%d" % Q)


SMALL_T = 8


def _small(Q, seed):
    rs = np.random.RandomState(seed)
    v = torch.from_numpy(rs.standard_normal((1, Q, SMALL_T)).astype(np.float32))
    t = torch.from_numpy(rs.randint(0, Q, size=(1, SMALL_T)).astype(np.int64))
    return v, t


def check_softmax_masked_target(Q, lib, device):
    """The TARGET at -1e30: a finite loss of about 1e30.  At -inf: loss +inf as torch gives, ``dlogits`` finite everywhere."""
    eng = op_engine(Q, lib, device)
    v, t = _small(Q, 4100 + Q)
    col = 5
    for fill in (-1e30, -float("inf")):
        vb = v.clone()
        vb[0, int(t[0, col]), col] = fill
        ref = softmax_refs(vb, t)
        live = live_mask(1, SMALL_T, 0)
        loss, dl = eng.loss(vb.to(device), t.to(device), 0, 1.0)
        want32 = torch.nn.functional.cross_entropy(vb, t)
        assert bool(torch.isfinite(dl).all()), fill
        if math.isinf(fill):
            assert float(loss.cpu()) == float("inf") and float(want32) == float("inf")
        else:
            assert math.isfinite(float(loss.cpu()))
            check_mean("softmax_ce Q=%d target at -1e30" % Q, loss, ref, live)
            assert abs(float(loss.cpu()) - 1e30 / SMALL_T) <= 1e-6 * 1e30
        check_softmax_grad("softmax_ce Q=%d target at %g" % (Q, fill), dl, ref, live, 1.0 / SMALL_T, ["P4"] * SMALL_T)


def check_softmax_nonfinite(Q, lib, device):
    """One NaN, and in another call one +inf, in one column: the loss and that column's ``dlogits`` are non-finite, every other
    column of ``dlogits`` has the bits of the same call without the bad value."""
    eng = op_engine(Q, lib, device)
    v, t = _small(Q, 4200 + Q)
    _, base = eng.loss(v.to(device), t.to(device), 0, 1.0)
    base = base.cpu().clone()
    col = 3
    for bad in (float("nan"), float("inf")):
        vb = v.clone()
        vb[0, (int(t[0, col]) + 1) % Q, col] = bad
        loss, dl = eng.loss(vb.to(device), t.to(device), 0, 1.0)
        dl = dl.cpu()
        assert not math.isfinite(float(loss.cpu())), bad
        assert not bool(torch.isfinite(dl[0, :, col]).any()), (bad, dl[0, :, col])
        keep = [c for c in range(SMALL_T) if c != col]
        assert torch.equal(dl[:, :, keep], base[:, :, keep]), bad


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fused epilogue of conv_post_2 (k_gemm6<CE = true, F16 = false / true>), through the head's parameters
# ---------------------------------------------------------------------------------------------------------------------
FUSED_CONFIGS = {256: (256, 6, 64, 128, 2, 1, 2, 16), 200: (200, 4, 64, 128, 2, 1, 2, 0), 130: (130, 4, 64, 128, 2, 1, 2, 0),
                 128: (128, 4, 64, 128, 2, 1, 2, 0)}
FUSED_B, FUSED_T = 2, 272               # a ragged last 128-column tile
FUSED_LENGTHS = (150, FUSED_T)          # one end inside the second tile
FUSED_GRAD_SCALE = 0.625
FUSED_FLAGS = {"default": DEFAULT_FLAGS, "six": SIX_PRODUCT_FLAGS}
W2, B2, B1 = "conv_post_2.weight", "conv_post_2.bias", "conv_post_1.bias"


def _rows_for(Q):
    """F2's placements of the dominant class: the two lane halves, another i, the other wave row, the last class."""
    return [r for r in (3, 7, 40, 133, Q - 1) if r < Q]


def fused_cases(Q):
    """name -> (family, function editing a copy of the parameters, class every target is moved to or None)."""
    def scale_w(f):
        def e(p):
            p[W2] = p[W2] * f
        return e

    def peak(row):
        def e(p):
            p[B2][row] += 50.0
            if row >= 128:
                other = row - 128
            elif Q > 128:
                other = row + 128 if row + 128 < Q else Q - 1
            else:
                other = (row + 64) % Q        # 128 classes: the second wave row is all padding
            p[B2][other] += 25.0              # a class of the other wave row (where there is one)
        return e

    def offset(o):
        def e(p):
            p[B2] += o
        return e

    def masked(p):
        p[B2][1] = p[B2][Q - 2] = -1e30
        p[B2][9] = p[B2][Q // 2 + 3] = -float("inf")

    def flat(kind):
        def e(p):
            p[W2] = torch.zeros_like(p[W2])
            p[B2] = torch.full_like(p[B2], -2.0)
            if kind == "all_equal":
                p[B2][:] = 0.5
            elif kind == "tie_halves":      # rows 3 and 7: the two lane halves of one wave
                p[B2][3] = p[B2][7] = 4.0
            elif kind == "tie_waves":       # row 2 and a row of the second wave row (or, with 128 classes, another i)
                p[B2][2] = p[B2][Q - 1] = 4.0
        return e

    cases = {"F0": ("F0", lambda p: None, None)}
    for f in (30.0, 100.0):
        cases["F1_x%d" % f] = ("F1", scale_w(f), None)
    for r in _rows_for(Q):
        cases["F2_row%d" % r] = ("F2", peak(r), None)
    for o in (3e4, -3e4):
        cases["F3_%+g" % o] = ("F3", offset(o), None)
    cases["F4_masked"] = ("F4", masked, None)
    for kind in ("all_equal", "tie_halves", "tie_waves"):
        cases["F5_" + kind] = ("F5", flat(kind), None)
    return cases


@functools.lru_cache(maxsize=None)
def fused_instance(Q):
    cfg_t = FUSED_CONFIGS[Q]
    cfg = O.OracleConfig(*cfg_t)
    assert cfg.receptive_field % 128 != 0
    params = O.random_params(cfg, 300 + Q, scale=0.3)
    x, h, t = O.synthetic_batch(cfg, FUSED_B, FUSED_T, 301 + Q)
    return cfg, params, x, h, t


def _off_the_masked(t, Q):
    """F4: the seeded targets moved off the four masked classes (the masked-TARGET runs put them there on purpose)."""
    t = t.clone()
    for q in (1, Q - 2, 9, Q // 2 + 3):
        t[t == q] = q + 1
    return t


def _fused_engine(Q, lib, device, flags, params):
    eng = WaveNetEngine(*FUSED_CONFIGS[Q], device=device, library=lib)
    eng.flags = flags
    load_state_into_flat(eng, params)
    assert eng.lib.wn_forward_loss_fused(ctypes.byref(eng.cfg), FUSED_B, FUSED_T, eng.flags) == 1, Q
    return eng


def check_fused(Q, arith, case, lib, device, worst=None):
    """One case of section 3 on one configuration and arithmetic: forward_loss, forward_loss(lengths=) and forward_nll against the
    fp64 softmax of the fp32 logits ``forward`` returns under the same flags; those logits against O.forward in fp64."""
    cfg, params, x, h, t = fused_instance(Q)
    family, edit, _ = fused_cases(Q)[case]
    p = {k: v.clone() for k, v in params.items()}
    edit(p)
    B, T, gs = FUSED_B, FUSED_T, FUSED_GRAD_SCALE
    rf = cfg.receptive_field
    if family == "F4":
        t = _off_the_masked(t, Q)
    eng = _fused_engine(Q, lib, device, FUSED_FLAGS[arith], p)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    logits = eng.forward(xd, hd).cpu()
    with torch.no_grad():
        l64 = O.forward(cfg, {k: v.double() for k, v in p.items()}, x, h.double()).transpose(1, 2)
    fin = torch.isfinite(l64)
    assert torch.equal(torch.isfinite(logits), fin) or family == "F4"
    big = l64.abs() < 1e29
    e_log = float((logits.double() - l64)[big].abs().max())
    print("fused Q=%d %s %s: logits err %.3g (max |logits_64| %.3g)" % (Q, arith, case, e_log, float(l64[big].abs().max())))
    assert e_log <= PC.TOL_LOGITS * max(1.0, float(l64[big].abs().max())), (Q, arith, case, e_log)
    ref = softmax_refs(logits, t)
    fam = [family] * T
    worst = Worst() if worst is None else worst
    tag = "fused Q=%d %s %s" % (Q, arith, case)
    for name, lengths in (("dense", None), ("ragged", list(FUSED_LENGTHS))):
        live = live_mask(B, T, rf, lengths)
        assert bool(torch.isfinite(ref["nll"][live]).all()), tag
        loss, dl = eng.forward_loss(xd, hd, td, grad_scale=gs, lengths=lengths)
        check_softmax_grad("%s %s" % (tag, name), dl, ref, live, gs / int(live.sum()), fam, worst)
        check_mean("%s %s" % (tag, name), loss, ref, live, worst)
        if family == "F4":
            masked = (logits <= -1e30) & live[:, None, :] & ~ref["hot"]
            assert bool(masked.any()) and float(dl.cpu()[masked].abs().max()) == 0.0, tag
            assert bool(torch.isfinite(dl).all()), tag
        if name == "ragged":   # (its second sequence runs to T: the dense rows are in it)
            row, counts = eng.forward_nll(xd, hd, target=td, lengths=lengths)
            assert counts == [int(live[b].sum()) for b in range(B)]
            check_rows("%s %s" % (tag, name), row, ref, live, worst)
    return worst


def check_fused_invariants(Q, arith, lib, device):
    """On the unedited head: the launch log shows the epilogue and no softmax_ce launch; ``want_grad=False`` returns the same loss
    bits; the ragged call with full lengths is bit-equal to the dense one; forward_nll without lengths is the dense rows."""
    cfg, params, x, h, t = fused_instance(Q)
    B, T, gs = FUSED_B, FUSED_T, FUSED_GRAD_SCALE
    eng = _fused_engine(Q, lib, device, FUSED_FLAGS[arith], params)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    box = {}
    log = PC.launch_log(eng.lib, lambda: box.update(r=eng.forward_loss(xd, hd, td, grad_scale=gs)))
    assert "fwd_post2_ce" in log and "softmax_ce" not in log, log
    loss, dl = box["r"]
    loss, dl = loss.cpu().clone(), dl.cpu().clone()
    loss0, none = eng.forward_loss(xd, hd, td, grad_scale=gs, want_grad=False)
    assert none is None and torch.equal(loss0.cpu(), loss)
    loss1, dl1 = eng.forward_loss(xd, hd, td, grad_scale=gs, lengths=[T] * B)
    assert torch.equal(loss1.cpu(), loss) and torch.equal(dl1.cpu(), dl)
    row, counts = eng.forward_nll(xd, hd, target=td)
    row1, counts1 = eng.forward_nll(xd, hd, target=td, lengths=[T] * B)
    assert counts == counts1 and torch.equal(row.cpu(), row1.cpu())
    ref = softmax_refs(eng.forward(xd, hd).cpu(), t)
    check_rows("fused Q=%d %s dense" % (Q, arith), row, ref, live_mask(B, T, cfg.receptive_field))


def check_fused_masked_target(Q, arith, lib, device):
    """F4 with a target among the masked classes: every target of sequence 0 moved to the class at -1e30 (a finite loss of
    about 1e30), every target of sequence 1 to a class at -inf (loss +inf, ``dlogits`` finite)."""
    cfg, params, x, h, t = fused_instance(Q)
    p = {k: v.clone() for k, v in params.items()}
    fused_cases(Q)["F4_masked"][1](p)
    B, T, gs, rf = FUSED_B, FUSED_T, FUSED_GRAD_SCALE, cfg.receptive_field
    eng = _fused_engine(Q, lib, device, FUSED_FLAGS[arith], p)
    xd, hd = x.to(device), h.to(device)
    logits = eng.forward(xd, hd).cpu()
    for name, cls, b_hit in (("-1e30", 1, 0), ("-inf", 9, 1)):
        t2 = _off_the_masked(t, Q)
        t2[b_hit, rf + 3::7] = cls
        ref = softmax_refs(logits, t2)
        live = live_mask(B, T, rf)
        loss, dl = eng.forward_loss(xd, hd, t2.to(device), grad_scale=gs)
        tag = "fused Q=%d %s target at %s" % (Q, arith, name)
        assert bool(torch.isfinite(dl).all()), tag
        check_softmax_grad(tag, dl, ref, live, gs / int(live.sum()), ["F4"] * T)
        row, _ = eng.forward_nll(xd, hd, target=t2.to(device))
        if name == "-inf":
            assert float(loss.cpu()) == float("inf") and float(row.cpu()[b_hit]) == float("inf"), tag
            assert math.isfinite(float(row.cpu()[1 - b_hit]))
        else:
            assert math.isfinite(float(loss.cpu())) and float(loss.cpu()) > 1e27, tag
            check_mean(tag, loss, ref, live)
            check_rows(tag, row, ref, live)


def check_fused_redo(Q, lib, device):
    """F6: under the fp16-pair flags relu(post1) beyond fp16's range (+1e5 on conv_post_1.bias): conv_post_2's first launch
    writes dlogits, the loss partials and the max-|dlogits| partials from non-finite accumulators, the conditional six-product
    launch must replace all three.  Loss, dlogits and row sums bit-equal to the six-product flag set and finite; backward with
    the workspace's max-|dlogits| word against backward with the scan forced."""
    cfg, params, x, h, t = fused_instance(Q)
    p = {k: v.clone() for k, v in params.items()}
    p[B1] = p[B1] + 1.0e5
    B, T, gs = FUSED_B, FUSED_T, FUSED_GRAD_SCALE
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    out = {}
    for name in ("six", "default"):
        eng = _fused_engine(Q, lib, device, FUSED_FLAGS[name], p)
        log = PC.launch_log(eng.lib, lambda: eng.forward_loss(xd, hd, td, grad_scale=gs))
        assert ("mm_redo_if_overflow" in log) == (name == "default"), log
        res = []
        for lengths in (None, list(FUSED_LENGTHS)):
            loss, dl = eng.forward_loss(xd, hd, td, grad_scale=gs, lengths=lengths)
            row, _ = eng.forward_nll(xd, hd, target=td, lengths=lengths)
            res += [loss.cpu().clone(), dl.cpu().clone(), row.cpu().clone()]
        out[name] = res
        if name == "default":
            loss, dl = eng.forward_loss(xd, hd, td, grad_scale=gs)
            g_word = eng.backward(dl).cpu().clone()                     # the workspace's max-|dlogits| word
            dl2 = dl.clone()
            eng.grads().fill_(float("nan"))
            g_scan = eng.backward(dl2, dlogits_bound=None).cpu().clone()   # another tensor object: the library scans it
            assert bool(torch.isfinite(g_word).all()) and bool(torch.isfinite(g_scan).all())
            gw = PC.flat_to_state(eng, g_word, O.param_shapes(cfg))
            gsn = PC.flat_to_state(eng, g_scan, O.param_shapes(cfg))
            for k in gw:
                e = PC.rel_to_max(gw[k], gsn[k])
                assert e <= PC.TOL_GRAD, (k, e)
    for a, b in zip(out["default"], out["six"]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), Q
    # and the redo's result is the right softmax of the logits the six-product forward returns
    eng = _fused_engine(Q, lib, device, FUSED_FLAGS["six"], p)
    ref = softmax_refs(eng.forward(xd, hd).cpu(), t)
    live = live_mask(B, T, cfg.receptive_field)
    check_softmax_grad("fused Q=%d redo" % Q, out["default"][1], ref, live, gs / int(live.sum()), ["F6"] * T)
    check_mean("fused Q=%d redo" % Q, out["default"][0], ref, live)


# ---------------------------------------------------------------------------------------------------------------------
# 4. mixture-of-logistics head at op level: wn_mol_loss, wn_mol_loss_ragged, wn_mol_nll_rows (k_mol_nll / mol_component)
# ---------------------------------------------------------------------------------------------------------------------
MOL_Y = (-1.0, -0.9995, -0.99, -0.3, 1e-3, 0.5, 0.99, 0.9995, 1.0)
MOL_DY = (0.0, 1e-5, -1e-5, 1e-3, -1e-3, 0.1, -0.1, 1.0, -1.0, 2.0, -2.0)
MOL_LS = (-30.0, -7.5, -7.0, -6.9, -5.0, -2.0, 0.0, 3.0)
MOL_GRID = len(MOL_Y) * len(MOL_DY) * len(MOL_LS)           # 792
MOL_T_START, MOL_T = 4, 800                                 # the grid on [4, 796), four random positions behind it
MOL_RAGGED = (MOL_T_START + MOL_GRID,)
MOL_REGIMES = ("normal3", "one_plus60", "tied")
MOL_CLASSES = (256, 65536)
MOL_NMIX = (1, 3, 10)
MOL_K = 16.0
MOL_LOG_SCALE_MIN = -7.0
MOL_GRAD_SCALE = 1.5
MOL_MAX_LEFT_OUT = 0.40
F32_0999 = float(np.float32(0.999))                         # the kernel compares y in fp32, and float32(0.999) != 0.999
assert MOL_GRID == 792 and MOL_T % MC.CFG[7] == 0


@functools.lru_cache(maxsize=None)
def mol_instance(nm, regime):
    """out (1, 3 nm, T) fp32 and y (1, T) fp32: component 0 of position 4 + g takes grid point g, the other components are
    random (means U(-1, 1), raw log-scales U(-8, 1)); the mixture logits follow ``regime``."""
    rs = np.random.RandomState(5000 + 10 * nm + MOL_REGIMES.index(regime))
    T = MOL_T
    y = rs.uniform(-1, 1, T).astype(np.float32)
    mean = rs.uniform(-1, 1, (nm, T)).astype(np.float32)
    ls = rs.uniform(-8, 1, (nm, T)).astype(np.float32)
    g = 0
    for yv in MOL_Y:
        for dy in MOL_DY:
            for l in MOL_LS:
                t = MOL_T_START + g
                y[t] = np.float32(yv)
                mean[0, t] = np.float32(y[t]) - np.float32(dy)
                ls[0, t] = np.float32(l)
                g += 1
    # The grid is component 0's; with ten components drawn freely, seven positions in ten have SOME component next to the branch
    # switch at 65536 classes (cdf_delta ~ 3e-5 x density, and a wide component's density is 0.2 - 0.6 over its whole middle).
    # So a random component whose own cdf_delta, at either class count, lies within a factor 4 of the band is drawn again.
    for _ in range(200):
        inv = np.exp(-np.maximum(ls[1:].astype(np.float64), MOL_LOG_SCALE_MIN))
        c = y.astype(np.float64)[None] - mean[1:].astype(np.float64)
        near = np.zeros(c.shape, dtype=bool)
        for classes in MOL_CLASSES:
            half = 1.0 / (classes - 1)
            with np.errstate(over="ignore"):
                delta = 1.0 / (1.0 + np.exp(-inv * (c + half))) - 1.0 / (1.0 + np.exp(-inv * (c - half)))
            near |= (delta > 0.125e-5) & (delta < 8e-5)
        if not near.any():
            break
        mean[1:][near] = rs.uniform(-1, 1, int(near.sum())).astype(np.float32)
        ls[1:][near] = rs.uniform(-8, 1, int(near.sum())).astype(np.float32)
    if regime == "normal3":
        logit = 3.0 * rs.standard_normal((nm, T))
    elif regime == "one_plus60":
        logit = rs.standard_normal((nm, T))
        logit[rs.randint(nm, size=T), np.arange(T)] += 60.0
    else:
        logit = np.full((nm, T), 0.25)
    out = np.concatenate([logit.astype(np.float32), mean, ls], axis=0)[None]
    return torch.from_numpy(out), torch.from_numpy(y)[None]


def mol_position_nll(out, y, num_classes, log_scale_min=MOL_LOG_SCALE_MIN):
    """The published formula as O.mol_nll states it, per position with no mean: out (B, T, 3 nm), y (B, T) -> (nll (B, T),
    cdf_delta (B, T, nm), A (B, T, nm), inv (B, T, nm)).  y against the fp32 values -0.999f / 0.999f."""
    nm = out.size(-1) // 3
    yy = y.unsqueeze(-1)
    logit, mean = out[..., :nm], out[..., nm:2 * nm]
    ls = torch.clamp(out[..., 2 * nm:3 * nm], min=log_scale_min)
    half = 1.0 / (num_classes - 1)
    inv = torch.exp(-ls)
    c = yy - mean
    plus_in, min_in, mid_in = inv * (c + half), inv * (c - half), inv * c
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    log_cdf_plus = plus_in - torch.nn.functional.softplus(plus_in)
    log_one_minus_cdf_min = -torch.nn.functional.softplus(min_in)
    log_pdf_mid = mid_in - ls - 2.0 * torch.nn.functional.softplus(mid_in) - float(np.log((num_classes - 1) / 2.0))
    inner = torch.where(cdf_delta > 1e-5, torch.log(torch.clamp(cdf_delta, min=1e-12)), log_pdf_mid)
    ll = torch.where(yy < -F32_0999, log_cdf_plus, torch.where(yy > F32_0999, log_one_minus_cdf_min, inner))
    lp = ll + torch.log_softmax(logit, dim=-1)
    return -torch.logsumexp(lp, dim=-1), cdf_delta.detach(), (inv * (c.abs() + half)).detach(), inv.detach()


def mol_refs(out, y, num_classes):
    """fp64 per-position nll and gradient (autograd on the SUM of the per-position values: positions are independent), the
    fp32 evaluation's errors against them, the scales of the gate and the positions left out of the numeric comparison."""
    res = {}
    for dt in (torch.float64, torch.float32):
        ri = out.transpose(1, 2).clone().to(dt).requires_grad_(True)
        nll, delta, A, inv = mol_position_nll(ri, y.to(dt), num_classes)
        nll.sum().backward()
        res[dt] = (nll.detach().double(), ri.grad.double(), delta.double(), A.double(), inv.double())
    nll, g, delta, A, inv = res[torch.float64]
    nm = A.size(-1)
    e_g = (res[torch.float32][1] - g).abs()
    e_g = torch.where(torch.isfinite(e_g), e_g, torch.zeros_like(e_g))
    e_nll = (res[torch.float32][0] - nll).abs()
    e_nll = torch.where(torch.isfinite(e_nll), e_nll, torch.zeros_like(e_nll))
    amax = A.amax(dim=-1, keepdim=True)
    S = torch.cat([torch.ones_like(A), inv, 1.0 + A], dim=-1)
    left_out = ((delta > 0.5e-5) & (delta < 2e-5)).any(dim=-1)          # (B, T)
    return dict(nll=nll, g=g, e_g=e_g, e_nll=e_nll, gate=FACTOR * e_g + MOL_K * U24 * S * (1.0 + amax),
                nll_gate=FACTOR * e_nll + MOL_K * U24 * (1.0 + nll.abs() + amax[..., 0]), left_out=left_out, nm=nm)


def c_mol_rows(eng, out, y, t_start, t_end, num_classes, acc=None):
    B, _, T = out.shape
    ws = eng.eval_workspace(B, T)
    row = torch.full((B,), float("nan"), dtype=torch.float32, device=out.device)
    rc = eng.lib.wn_mol_nll_rows(ctypes.byref(eng.cfg), B, T, _ptr(out), _ptr(y), int(t_start), _ptr(t_end), int(num_classes),
                                 float(MOL_LOG_SCALE_MIN), _ptr(row), _ptr(acc), _ptr(ws), ws.numel() * 4, _stream_handle(eng.device))
    assert rc == 0, eng.lib.wn_last_error().decode()
    return row


def check_mol_op(num_classes, nm, regime, lib, device):
    out, y = mol_instance(nm, regime)
    ref = mol_refs(out, y, num_classes)
    T, ts, gs = MOL_T, MOL_T_START, MOL_GRAD_SCALE
    eng = WaveNetEngine(*MC.CFG, device=device, library=lib, out_channels=3 * nm)
    od, yd = out.to(device), y.to(device)
    tag = "mol classes=%d nm=%d %s" % (num_classes, nm, regime)
    # computed from the reference alone: at most 40 % of the positions of a call sit next to the formula's branch switch
    grid = slice(ts, ts + MOL_GRID)
    n_out = int(ref["left_out"][0, grid].sum())
    print("%s: %d of %d grid positions left out (fp64 cdf_delta of a component in (0.5e-5, 2e-5))" % (tag, n_out, MOL_GRID))
    assert n_out <= MOL_MAX_LEFT_OUT * MOL_GRID, (tag, n_out)
    kind = ["logit"] * nm + ["mean"] * nm + ["log_scale"] * nm
    worst = Worst()
    dense = None
    for name, lengths in (("dense", None), ("ragged", list(MOL_RAGGED)), ("full", [T])):
        live = live_mask(1, T, ts, lengths)
        n = int(live.sum())
        kw = dict(t_start=ts, grad_scale=gs, num_classes=num_classes, log_scale_min=MOL_LOG_SCALE_MIN, lengths=lengths)
        loss, dout = eng.mol_loss(od, yd, **kw)
        loss0, none = eng.mol_loss(od, yd, want_grad=False, **kw)
        assert none is None and torch.equal(loss0.cpu(), loss.cpu()), tag
        if name == "dense":
            dense = (loss.cpu().clone(), dout.cpu().clone())
        if name == "full":
            assert torch.equal(loss.cpu(), dense[0]) and torch.equal(dout.cpu(), dense[1]), tag
            continue
        dk = dout.cpu().transpose(1, 2)                                   # (1, T, 3 nm)
        assert bool(torch.isfinite(dk).all()) and math.isfinite(float(loss.cpu())), tag
        assert float(dk[~live].abs().max()) == 0.0, tag                   # zeros outside the live positions
        raw = out.transpose(1, 2)[..., 2 * nm:]
        below = (raw < MOL_LOG_SCALE_MIN) & live[..., None]
        assert bool(below.any()) and float(dk[..., 2 * nm:][below].abs().max()) == 0.0, tag   # clamped: exactly zero
        if nm == 1:
            assert float(dk[..., 0].abs().max()) == 0.0, tag              # one component: d(logit) is exactly 0
        err = (dk.double() / (gs / n) - ref["g"]).abs()
        judged = live & ~ref["left_out"]
        frac = err / ref["gate"]
        bad = []
        for t in torch.nonzero(judged[0]).reshape(-1).tolist():
            for j in range(3 * nm):
                worst.note(kind[j], "d", float(err[0, t, j]), float(ref["e_g"][0, t, j]), float(frac[0, t, j]))
            if float(frac[0, t].max()) > 1.0:
                j = int(frac[0, t].argmax())
                bad.append("%s %s t=%d (y=%.6g, out=%s) %s %d: err %.3g > gate %.3g (fp32 formula: %.3g), k needed %.1f"
                           % (tag, name, t, float(y[0, t]), [float(out[0, i * nm, t]) for i in range(3)] if j % nm == 0 else "..",
                              kind[j], j % nm, float(err[0, t, j]), float(ref["gate"][0, t, j]), float(ref["e_g"][0, t, j]),
                              MOL_K * float((err[0, t, j] - FACTOR * ref["e_g"][0, t, j]) / (ref["gate"][0, t, j] - FACTOR * ref["e_g"][0, t, j]))))
        assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])
        # a raw log-scale exactly at log_scale_min passes its gradient, as torch.clamp does
        at = (raw[..., 0] == MOL_LOG_SCALE_MIN) & judged & (ref["g"][..., 2 * nm].abs() > 1e-3)
        assert bool(at.any()) and bool((dk[..., 2 * nm][at] != 0.0).all()), tag
    # every position's own value (sequences of one live position, as for the softmax head), and the sums against them
    U = MC.CFG[7]
    o1 = torch.zeros((T, 3 * nm, U), dtype=torch.float32)
    o1[:, :, 0] = out[0].transpose(0, 1)
    y1 = torch.zeros((T, U), dtype=torch.float32)
    y1[:, 0] = y[0]
    ones = torch.ones(T, dtype=torch.int32).to(device)
    nll_k = c_mol_rows(eng, o1.to(device), y1.to(device), 0, ones, num_classes).cpu().double()[None]
    assert bool(torch.isfinite(nll_k).all()), tag
    e = (nll_k - ref["nll"]).abs()
    judged = ~ref["left_out"]
    for t in torch.nonzero(judged[0]).reshape(-1).tolist():
        worst.note("nll", "nll", float(e[0, t]), float(ref["e_nll"][0, t]), float(e[0, t] / ref["nll_gate"][0, t]))
    bad = ["%s t=%d: |nll_k - nll_64| = %.3g > %.3g (nll_64 %.6g)" % (tag, t, float(e[0, t]), float(ref["nll_gate"][0, t]), float(ref["nll"][0, t]))
           for t in range(T) if bool(judged[0, t]) and not float(e[0, t]) <= float(ref["nll_gate"][0, t])]
    assert not bad, "\n".join(bad[:12] + ["... %d failures" % len(bad)])
    for lengths in (None, list(MOL_RAGGED)):
        live = live_mask(1, T, ts, lengths)
        t_end = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).to(device)
        row = c_mol_rows(eng, od, yd, ts, t_end, num_classes)
        acc = torch.full((1,), -3.0, dtype=torch.float64, device=device)
        row_a = c_mol_rows(eng, od, yd, ts, t_end, num_classes, acc)
        assert torch.equal(row.cpu(), row_a.cpu()) and abs(float(acc.cpu()) + 3.0 - float(row.cpu().double().sum())) <= 1e-9
        own = float(nll_k[live].sum())
        slack = 2.0 ** -22 * float(nll_k[live].abs().sum())
        assert abs(float(row.cpu()[0]) - own) <= slack, (tag, float(row.cpu()[0]), own)
        loss, _ = eng.mol_loss(od, yd, t_start=ts, num_classes=num_classes, log_scale_min=MOL_LOG_SCALE_MIN, lengths=lengths, want_grad=False)
        assert abs(float(loss.cpu()) - own / int(live.sum())) <= slack / int(live.sum()), tag
    worst.report(tag)


# ---------------------------------------------------------------------------------------------------------------------
# the case matrices of the two test files
# ---------------------------------------------------------------------------------------------------------------------
FUSED_MATRIX = [(Q, a, c) for Q in FUSED_CONFIGS for a in FUSED_FLAGS for c in fused_cases(Q)]
# The host emulator runs a forward pass of these configurations in ~3 s and a case takes four: it visits every case, every
# configuration, both arithmetics and every placement of the maximum once, not their product (the MI355X file runs the product).
FUSED_MATRIX_EMU = [
    (256, "default", "F0"), (256, "six", "F2_row133"), (256, "default", "F2_row255"), (256, "six", "F5_tie_waves"),
    (256, "default", "F3_+30000"), (200, "six", "F1_x100"), (200, "default", "F2_row3"), (200, "six", "F2_row7"),
    (200, "default", "F4_masked"), (200, "six", "F3_-30000"), (130, "default", "F1_x30"), (130, "six", "F2_row129"),
    (130, "default", "F5_tie_waves"), (128, "six", "F0"), (128, "default", "F2_row40"), (128, "six", "F5_all_equal"),
    (128, "default", "F5_tie_halves"),
]
assert set(FUSED_MATRIX_EMU) <= set(FUSED_MATRIX)
assert {fused_cases(Q)[c][0] for Q, _, c in FUSED_MATRIX_EMU} == {"F0", "F1", "F2", "F3", "F4", "F5"}
assert {(Q, a) for Q, a, _ in FUSED_MATRIX_EMU} == {(Q, a) for Q in FUSED_CONFIGS for a in FUSED_FLAGS}
assert {c for _, _, c in FUSED_MATRIX_EMU} >= {"F2_row3", "F2_row7", "F2_row40", "F2_row133", "F2_row255", "F5_all_equal",
                                               "F5_tie_halves", "F5_tie_waves"}
MOL_MATRIX = [(c, nm, r) for c in MOL_CLASSES for nm in MOL_NMIX for r in MOL_REGIMES]
