# -*- coding: utf-8 -*-
"""Layer-wise adaptive steps (LAMB) in FusedAdam and per-tensor norms (wn_tensor_table / wn_lamb_step /
wn_tensor_sumsq, ``FusedAdam(layer_adaptation=True)``): the cases tests/test_emu_lamb.py runs on the host-compiled kernels and
tests/test_gpu_lamb.py on the MI355X.

The reference (``ref_step``) is an fp64 restatement of the contract in include/wavenet_hip.h, fed the same fp32 inputs as the
library; every element of every tensor is checked.  Tolerances:
  weights   |w - w_ref| <= PC.TOL_ADAM_REL_LR * lr_g * r_ref,k + 2^-23 |w_ref|: the project's Adam gate scaled to the tensor's
            step, plus the rounding of the stored weight;
  moments   CC.MOMENT_TOL of the maximum, and bit-identity with the grouped Adam launch;
  ratio and norms   1e-5 relative (u has at most six fp32 roundings, about 4e-7; the sums are in double);
  tensor_sumsq      1e-12 relative against numpy fp64.
"""
import ctypes

import numpy as np
import torch

from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import clip_common as CC
from tests import freeze_common as FC
from tests import groups_common as GC
from tests import parity_common as PC

TINY = CC.TINY
LR = 1e-3
BETAS = (0.9, 0.999)
C = _lib.TENSOR_CHUNK
STAT_TOL = 1e-5
SUMSQ_TOL = 1e-12
# (lr, eps, weight_decay, decoupled): no decay, L2, decoupled
G3 = [(LR, 1e-8, 0.0, 0), (3.0 * LR, 1e-6, 1e-2, 0), (0.3 * LR, 1e-8, 1e-1, 1)]
VARIANTS = FC.VARIANTS
bits = FC.bits


# ---- layouts: (lo, hi, group, adapt) per tensor and the buffer length --------------------------------------------------------------
def _lay(lens, groups, adapt, gap_after):
    quads, lo = [], 2
    for i, (ln, g, a) in enumerate(zip(lens, groups, adapt)):
        quads.append((lo, lo + ln, g, a))
        lo += ln + gap_after.get(i, 0)
    return quads, lo + 3


def layout_chunks():
    """Lengths 1, 3, C - 1, C, C + 1 and 2 C + 3 (a multi-block tensor, the order of its partials, head and tail), an adapted tensor
    between two that do not adapt, a multi-block tensor that does not adapt, groups sharing a tensor boundary, two gaps."""
    lens = [1, 3, C - 1, C, C + 1, 2 * C + 3, 5, 7, 9, C + 5]
    return _lay(lens, [0, 1, 0, 1, 2, 0, 1, 1, 2, 2], [1, 1, 1, 1, 1, 1, 0, 1, 0, 0], {1: 2, 4: 3})


def layout_many():
    """1100 tensors of 1 to 3 elements: more ranges than the optimizer's other kernels stage in LDS."""
    k = 1100
    return _lay([1 + i % 3 for i in range(k)], [i % 3 for i in range(k)], [int(i % 4 != 1) for i in range(k)],
                {i: 1 + i % 2 for i in range(0, k, 7)})


LAYOUTS = {"chunks": layout_chunks, "many": layout_many}


def make_tensor_table(lib, dev, quads, n, n_groups):
    """(device table, n_ranges, n_live, scratch) through wn_tensor_table, its words checked against a numpy restatement."""
    nr = len(quads)
    flat = (ctypes.c_int64 * (4 * nr))(*[x for q in quads for x in q])
    host = torch.full((7 * nr + 1 + n // C,), -1, dtype=torch.int64)
    n_live = lib.wn_tensor_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, n_groups, ctypes.c_void_p(host.data_ptr()))
    assert n_live == sum(q[1] - q[0] for q in quads), lib.wn_last_error()
    lo, hi = np.array([q[0] for q in quads]), np.array([q[1] for q in quads])
    nb = (hi - lo + C - 1) // C
    want = np.concatenate([lo, hi, np.cumsum(hi - lo) - (hi - lo), [q[2] for q in quads], [q[3] for q in quads], np.cumsum(nb) - nb,
                           [nb.sum()], np.repeat(np.arange(nr), nb)])
    assert np.array_equal(host.numpy()[:len(want)], want) and bool((host[len(want):] == -1).all())   # (nothing written behind it)
    host = host[:len(want)]
    blocks = int(lib.wn_tensor_blocks(ctypes.c_void_p(host.data_ptr()), nr))
    assert blocks == int(nb.sum()) and int(lib.wn_lamb_scratch_floats(blocks)) == 4 * blocks
    scratch = torch.full((4 * blocks,), float("nan"), dtype=torch.float32, device=dev)   # (what it held must not matter)
    return host.to(dev), nr, int(n_live), scratch


def check_tensor_table(lib):
    make_tensor_table(lib, "cpu", layout_chunks()[0], layout_chunks()[1], 3)
    make_tensor_table(lib, "cpu", [(0, 10, 2, 1), (10, 20, 0, 0), (50, 100, 2, 1)], 100, 3)

    def error(quads, n=100, n_groups=3, null=None):
        nr = len(quads)
        flat = (ctypes.c_int64 * max(4 * nr, 1))(*[x for q in quads for x in q])
        host = torch.zeros(7 * nr + 1 + max(n, 0) // C, dtype=torch.int64)
        rc = lib.wn_tensor_table(None if null == "quads" else ctypes.cast(flat, ctypes.c_void_p), nr, n, n_groups,
                                 None if null == "table" else ctypes.c_void_p(host.data_ptr()))
        msg = lib.wn_last_error().decode()
        assert rc == -1 and "wn_tensor_table" in msg, (quads, rc, msg)
        return msg

    assert "NULL" in error([(0, 4, 0, 1)], null="quads") and "NULL" in error([(0, 4, 0, 1)], null="table")
    assert "empty table" in error([])
    assert "n <= 0" in error([(0, 4, 0, 1)], n=0)
    assert "sorted and disjoint" in error([(10, 20, 0, 1), (0, 5, 0, 1)]) and "sorted and disjoint" in error([(0, 10, 0, 1), (9, 20, 1, 1)])
    assert "outside" in error([(0, 10, 0, 1), (90, 101, 0, 1)]) and "outside" in error([(-1, 10, 0, 1)])
    assert "is empty" in error([(5, 5, 0, 1)]) and "is empty" in error([(7, 3, 0, 1)])
    assert "group" in error([(0, 4, 3, 1)]) and "group" in error([(0, 4, -1, 1)])
    assert "n_groups" in error([(0, 4, 0, 1)], n_groups=0) and "n_groups" in error([(0, 4, 0, 1)], n_groups=17)
    assert "adapt" in error([(0, 4, 0, 2)])
    assert lib.wn_tensor_blocks(None, 1) == -1 and "wn_tensor_blocks" in lib.wn_last_error().decode()


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------------
def ema_weight(decay, warm, t):
    d = min(decay, (1.0 + t) / (10.0 + t)) if warm else decay
    return float(np.float32(1.0 - d))


def ref_step(p, g, m, v, e, quads, vals, t, betas=BETAS, coef=1.0, max_trust=None, w=None):
    """One step in float64 from fp32 inputs (numpy arrays over the whole buffer).  Returns p, m, v, e (float64; untouched outside
    the ranges) and per tensor (wn, un, r)."""
    p, g, m, v = (np.asarray(a, np.float64).copy() for a in (p, g, m, v))
    e = None if e is None else np.asarray(e, np.float64).copy()
    b1, b2 = float(np.float32(betas[0])), float(np.float32(betas[1]))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    stats = []
    for lo, hi, gi, adapt in quads:
        lr, eps, wd = (float(np.float32(x)) for x in vals[gi][:3])
        dec = bool(vals[gi][3])
        s = slice(lo, hi)
        ghat = coef * g[s]
        if not dec:
            ghat = ghat + wd * p[s]
        m[s] = b1 * m[s] + (1.0 - b1) * ghat
        v[s] = b2 * v[s] + (1.0 - b2) * ghat * ghat
        u = (m[s] / bc1) / (np.sqrt(v[s]) / np.sqrt(bc2) + eps)
        if adapt:
            if dec:
                u = u + wd * p[s]
            wn, un = float(np.sqrt(np.sum(p[s] ** 2))), float(np.sqrt(np.sum(u ** 2)))
            r = wn / un if wn > 0.0 and un > 0.0 else 1.0
            if max_trust is not None:
                r = min(r, float(np.float32(max_trust)))
            p[s] = p[s] - lr * r * u
            stats.append((wn, un, r))
        else:   # plain Adam, decoupled as torch.optim.AdamW
            p[s] = (p[s] * (1.0 - lr * wd) if dec else p[s]) - lr * u
            stats.append((0.0, 0.0, 1.0))
        if e is not None:
            e[s] = e[s] + w * (p[s] - e[s])
    return p, m, v, e, np.array(stats)


def assert_step(what, quads, vals, got, ref, stats, stats_ref, e_steps=1):
    """Every element of every tensor against the reference, and the three statistics."""
    (p, m, v, e), (pr, mr, vr, er) = got, ref
    assert stats.shape == stats_ref.shape
    for k, (lo, hi, gi, adapt) in enumerate(quads):
        s = slice(lo, hi)
        lr = float(np.float32(vals[gi][0]))
        tol = PC.TOL_ADAM_REL_LR * lr * stats_ref[k, 2] + 2.0 ** -23 * np.abs(pr[s])
        err = np.abs(p[s].astype(np.float64) - pr[s])
        assert np.all(err <= tol), what + (k, "weights", float(err.max()), float(tol.min()))
        for ours, theirs, name in ((m, mr, "m"), (v, vr, "v")):
            assert np.max(np.abs(ours[s] - theirs[s])) <= CC.MOMENT_TOL * np.max(np.abs(theirs[s])), what + (k, name)
        if er is not None:   # one rounding of w and one of the fma on top of the weight's error
            assert np.all(np.abs(e[s] - er[s]) <= tol + 2.0 ** -22 * np.abs(er[s])), what + (k, "ema")
        for j, name in enumerate(("weight norm", "update norm", "ratio")):
            assert abs(stats[k, j] - stats_ref[k, j]) <= STAT_TOL * abs(stats_ref[k, j]), what + (k, name, stats[k, j], stats_ref[k, j])


# ---- op level ----------------------------------------------------------------------------------------------------------------------
def lamb_step(lib, dev, bufs, table, vals, step=1, state=None, max_trust=0.0, decay=0.999, warm=1, stats=None, betas=BETAS, ema=True):
    p, g, m, v, e = bufs
    tab, nr, n_live, scratch = table
    stats = torch.full((3 * nr,), -7.0, dtype=torch.float32, device=dev) if stats is None else stats
    arr = GC.group_array(vals)
    rc = lib.wn_lamb_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e) if ema else None, p.numel(), _ptr(tab), nr, n_live, step,
                          ctypes.cast(arr, ctypes.c_void_p), len(vals), betas[0], betas[1], float(max_trust), _ptr(state), decay, warm,
                          _ptr(scratch), _ptr(stats), _stream_handle(torch.device(dev)))
    lib.check(rc, "wn_lamb_step")
    return stats


def _inputs(n, quads, seed, zero_moments=False):
    rs = np.random.RandomState(seed)
    f = lambda a: np.asarray(a, np.float32)   # noqa: E731
    p, e, g = f(rs.standard_normal(n)), f(rs.standard_normal(n)), f(rs.standard_normal(n))
    m, v = f(0.1 * rs.standard_normal(n)), f(0.01 * rs.uniform(size=n))
    if zero_moments:
        m[:], v[:] = 0.0, 0.0
    live = FC.live_mask(n, [(q[0], q[1]) for q in quads]).numpy()
    for buf in (g, m, v):   # what lies outside every tensor is never read
        buf[~live] = np.nan
    return [p, g, m, v, e], live


def _to_dev(arrays, misalign, dev):
    mis = misalign if isinstance(misalign, tuple) else (misalign,) * 5
    return [FC._misaligned(torch.from_numpy(a), k, dev) for a, k in zip(arrays, mis)]


def check_lamb_step(lib, dev, layout, misalign, t=3, variants=VARIANTS, max_trust=None):
    """The four variants over one layout: against fp64; the moments of every tensor and everything of a tensor that does not
    adapt bit for bit the grouped Adam launch's; the same call twice the same bits; nothing outside the tensors touched (NaN in
    the gradient and the moments there); the gradient never written."""
    quads, n = LAYOUTS[layout]()
    table = make_tensor_table(lib, dev, quads, n, len(G3))
    tab, nr, n_live, _ = table
    src, live = _inputs(n, quads, 11 + t)
    live_t, dead_t = torch.from_numpy(live), torch.from_numpy(~live)
    plain = torch.zeros(n, dtype=torch.bool)
    for lo, hi, _, adapt in quads:
        plain[lo:hi] = not adapt
    max_norm = 0.5 * FC.live_norm64(torch.from_numpy(src[1]), [(q[0], q[1]) for q in quads])
    decay, warm = 0.999, 1
    for variant in variants:
        what = (layout, misalign, t, variant)
        guarded, ema = "guarded" in variant, "ema" in variant
        state = block = None
        coef = 1.0
        if guarded:
            g_dev = _to_dev(src, misalign, dev)[1]
            state = CC.new_state(dev)
            state[3] = t - 1
            state, block = GC.run_norm_groups(lib, dev, g_dev, (tab, nr, n_live), G3, max_norm=max_norm, guard=True, state=state)
            st = CC.read_state(state)
            assert st.apply == 1 and st.steps_applied == t and st.clip_coef < 1.0
            coef = min(1.0, max_norm / (FC.live_norm64(torch.from_numpy(src[1]), [(q[0], q[1]) for q in quads]) + 1e-6))
        runs = []
        for _ in range(2):
            a = _to_dev(src, misalign, dev)
            stats = lamb_step(lib, dev, a, table, G3, step=t, state=state, max_trust=max_trust or 0.0, decay=decay, warm=warm, ema=ema)
            runs.append([bits(x) for x in a] + [bits(stats)])
        assert all(torch.equal(x, y) for x, y in zip(*runs)), what + ("run to run",)
        b = _to_dev(src, misalign, dev)   # the grouped Adam launch on the same inputs (the table's first rows are a group table)
        GC.adam_groups(lib, dev, variant, *b, (tab, nr, n_live), G3, state, block, t, decay, warm)
        for x, y, x0, name in zip(a, b, src, "pgmve"):
            x0b = torch.from_numpy(x0).view(torch.int32)
            assert torch.equal(bits(x)[dead_t], x0b[dead_t]), what + (name, "outside the tensors")
            if name in "mv":
                assert torch.equal(bits(x)[live_t], bits(y)[live_t]), what + (name, "moments are the grouped launch's")
            if name in "pe":
                assert torch.equal(bits(x)[plain], bits(y)[plain]), what + (name, "a tensor that does not adapt")
        assert torch.equal(bits(a[1]), torch.from_numpy(src[1]).view(torch.int32)), what + ("g written",)
        assert torch.equal(bits(a[4]), torch.from_numpy(src[4]).view(torch.int32)) == (not ema)
        adapted = live_t & ~plain
        assert not torch.equal(bits(a[0])[adapted], bits(b[0])[adapted])   # not vacuous: an adapted tensor's step is not Adam's
        ref = ref_step(*src[:4], src[4] if ema else None, quads, G3, t, coef=coef, max_trust=max_trust, w=ema_weight(decay, warm, t))
        got = [x.cpu().numpy() for x in (a[0], a[2], a[3], a[4])]
        sg = stats.cpu().numpy().reshape(nr, 3).astype(np.float64)
        assert_step(what, quads, G3, got, ref[:4], sg, ref[4])
        if max_trust is not None:   # the clamp is exactly min(): some ratios sit on it, the others are untouched
            free = lamb_step(lib, dev, _to_dev(src, misalign, dev), table, G3, step=t, state=state, decay=decay, warm=warm, ema=ema)
            free = free.cpu().view(nr, 3)
            want = torch.minimum(free[:, 2], torch.tensor(max_trust, dtype=torch.float32))
            assert torch.equal(bits(stats.view(nr, 3)[:, 2]), bits(want)) and bool((free[:, 2] > max_trust).any()) \
                and bool((free[:, 2] < max_trust).any()), what


def check_guard_writes_nothing(lib, dev):
    """A guarded step with a NaN in a live gradient writes nothing: weights, moments, average and the statistics stay."""
    quads, n = layout_chunks()
    table = make_tensor_table(lib, dev, quads, n, len(G3))
    tab, nr, n_live, _ = table
    for idx in (quads[0][0], quads[5][0] + C + 1, quads[6][0]):   # an adapted tensor, its second block, a tensor that does not adapt
        src, _ = _inputs(n, quads, 5)
        src[1][idx] = np.nan
        a = _to_dev(src, 1, dev)
        state = CC.new_state(dev)
        state[3] = 4
        state, _ = GC.run_norm_groups(lib, dev, a[1], (tab, nr, n_live), G3, max_norm=1.0, guard=True, state=state)
        st = CC.read_state(state)
        assert st.apply == 0 and st.steps_skipped == 1 and st.steps_applied == 4
        for ema in (False, True):
            stats = torch.full((3 * nr,), -7.0, dtype=torch.float32, device=dev)
            before = [bits(x) for x in a]
            lamb_step(lib, dev, a, table, G3, state=state, stats=stats, ema=ema)
            assert all(torch.equal(bits(x), x0) for x, x0 in zip(a, before)), (idx, ema)
            assert bool((stats == -7.0).all()), (idx, ema, "stats written")


def check_zero_rules(lib, dev):
    """A zero tensor gets r = 1 and moves by lr u; zero gradient, zero moments and no decay leave p unchanged bit for bit, r = 1."""
    quads, n = _lay([C + 3, 5, 300], [0, 0, 0], [1, 1, 1], {0: 1})
    vals = [(LR, 1e-8, 0.0, 0)]
    table = make_tensor_table(lib, dev, quads, n, 1)
    nr = len(quads)
    src, _ = _inputs(n, quads, 9)
    (a0, a1, _, _), (b0, b1, _, _), _ = quads
    src[0][a0:a1] = 0.0                                     # tensor 0: zero weights
    for buf in src[1:4]:
        buf[b0:b1] = 0.0                                    # tensor 1: zero gradient and zero moments
    a = _to_dev(src, 2, dev)
    stats = lamb_step(lib, dev, a, table, vals, step=2, ema=False).cpu().view(nr, 3)
    assert stats[0, 0] == 0.0 and stats[0, 1] > 0.0 and stats[0, 2] == 1.0
    assert stats[1, 0] > 0.0 and stats[1, 1] == 0.0 and stats[1, 2] == 1.0
    assert torch.equal(bits(a[0])[b0:b1], torch.from_numpy(src[0]).view(torch.int32)[b0:b1])
    ref = ref_step(*src[:4], None, quads, vals, 2)
    assert_step(("zero rules",), quads, vals, [x.cpu().numpy() for x in (a[0], a[2], a[3], a[4])], ref[:4],
                stats.numpy().astype(np.float64), ref[4])
    assert float(np.abs(a[0].cpu().numpy()[a0:a1]).max()) > 0.0   # it moved: by lr * u (r = 1), as the reference says


def check_tensor_sumsq(lib, dev, layout, misalign):
    quads, n = LAYOUTS[layout]()
    tab, nr, n_live, scratch = make_tensor_table(lib, dev, quads, n, 3)
    x = CC.buffer(n, misalign, dev, seed=3)
    x64 = x.cpu().numpy().astype(np.float64)
    # magnitudes across the fp32 range, and what lies outside the ranges must not be read into any sum
    scale = np.where(np.arange(n) % 5 == 0, 1e18, np.where(np.arange(n) % 7 == 0, 1e-18, 1.0))
    x.copy_(torch.from_numpy((x64 * scale).astype(np.float32)))
    live = FC.live_mask(n, [(q[0], q[1]) for q in quads])
    x[(~live).to(dev)] = float("nan")
    out = torch.full((nr,), -1.0, dtype=torch.float64, device=dev)
    lib.check(lib.wn_tensor_sumsq(_ptr(x), n, _ptr(tab), nr, n_live, _ptr(scratch), _ptr(out), _stream_handle(torch.device(dev))),
              "wn_tensor_sumsq")
    x64 = x.cpu().numpy().astype(np.float64)
    want = np.array([np.sum(x64[lo:hi] ** 2) for lo, hi, _, _ in quads])
    got = out.cpu().numpy()
    assert np.all(np.abs(got - want) <= SUMSQ_TOL * want), (layout, misalign, float(np.max(np.abs(got - want) / want)))


def check_call_errors(lib, dev):
    quads, n = [(0, 10, 0, 1), (10, 20, 1, 0), (50, 100, 0, 1)], 100
    tab, nr, n_live, scratch = make_tensor_table(lib, dev, quads, n, 2)
    p, g, m, v, e = (torch.zeros(n, device=dev) for _ in range(5))
    stats, out = torch.zeros(3 * nr, device=dev), torch.zeros(nr, dtype=torch.float64, device=dev)
    state = CC.new_state(dev)
    st = _stream_handle(torch.device(dev))
    arr = GC.group_array(G3[:2])
    ap = ctypes.cast(arr, ctypes.c_void_p)
    odd = torch.zeros(4 * 8 + 1, device=dev)[1:]   # 4-byte aligned only
    assert odd.data_ptr() % 8 == 4

    def lamb(p_=p, tab_=tab, nl=n_live, step=1, groups=ap, ng=2, trust=0.0, state_=None, e_=None, decay=0.9, scratch_=scratch,
             stats_=stats):
        return lib.wn_lamb_step(_ptr(p_), _ptr(g), _ptr(m), _ptr(v), _ptr(e_), n, _ptr(tab_), nr, nl, step, groups, ng, 0.9, 0.999, trust,
                                _ptr(state_), decay, 1, _ptr(scratch_), _ptr(stats_), st)

    def sumsq(x_=g, tab_=tab, nl=n_live, scratch_=scratch, out_=out):
        return lib.wn_tensor_sumsq(_ptr(x_), n, _ptr(tab_), nr, nl, _ptr(scratch_), _ptr(out_), st)

    assert lamb() == 0 and lamb(e_=e) == 0 and lamb(trust=2.0) == 0 and lamb(state_=state, step=0) == 0 and sumsq() == 0

    def fails(rc, text):
        assert rc != 0 and text in lib.wn_last_error().decode(), (rc, text, lib.wn_last_error())

    fails(lamb(p_=None), "wn_lamb_step")
    fails(lamb(step=0), "wn_lamb_step")
    fails(lamb(tab_=None), "table is NULL")
    fails(lamb(nl=0), "n_live")
    fails(lamb(nl=n + 1), "n_live")
    fails(lamb(groups=None), "groups is NULL")
    fails(lamb(ng=0), "n_groups")
    fails(lamb(ng=17), "n_groups")
    fails(lamb(trust=-1.0), "max_trust")
    fails(lamb(trust=float("nan")), "max_trust")
    fails(lamb(scratch_=None), "scratch or stats is NULL")
    fails(lamb(stats_=None), "scratch or stats is NULL")
    fails(lamb(scratch_=odd), "alignment")
    fails(lamb(e_=p), "overlaps")
    fails(lamb(e_=e, decay=1.0), "ema_decay")
    fails(sumsq(x_=None), "wn_tensor_sumsq")
    fails(sumsq(out_=None), "wn_tensor_sumsq")
    fails(sumsq(tab_=None), "table is NULL")
    fails(sumsq(nl=0), "n_live")
    fails(sumsq(scratch_=odd), "alignment")
    eng = WaveNetEngine(*TINY, device=dev, library=lib)
    for bad, ng in (([], 2), ([(0, 5, 2, 1)], 2), ([(0, 5, 0, 3)], 1), ([(10, 20, 0, 1), (0, 5, 0, 1)], 2), ([(5, 5, 0, 1)], 1)):
        try:
            eng.tensor_table(bad, ng)
        except _lib.WnError as err:
            assert "wn_tensor_table" in str(err)
        else:
            raise AssertionError("tensor_table(%r) did not raise" % (bad,))


# ---- module level ------------------------------------------------------------------------------------------------------------------
GROUPS = [(r"bias$", {"lr": 3e-3, "weight_decay": 0.0}),
          (r"^conv_post|skip_1x1", {"lr": 1e-4, "weight_decay": 0.1, "decoupled_weight_decay": True, "eps": 1e-6})]
BASE = dict(lr=1e-3, weight_decay=1e-2, eps=1e-8)


def _adapts(opt, name, shape, gi):
    flag = opt.param_groups[gi].get("layer_adaptation")
    return len(shape) >= 2 if flag is None else flag


def check_module(lib, dev, case=None, clip=False, ema=False, freeze=None, groups=None, scheduler=False, accum=False, steps=3,
                 max_trust=None):
    """FusedAdam(layer_adaptation=True) against the fp64 reference, step by step: every step is compared from the library's own
    pre-step weights, moments and average and the gradient it produced, so the optimizer alone is judged."""
    cfg, model, _, (xd, hd, td), _ = GC._model(lib, dev, case)
    if freeze:
        assert model.freeze(freeze) > 0
    eng = model.engine
    model.loss_and_backward(xd, hd, td)
    live0 = [(off, off + n) for (off, n, shape, dead), p in zip(model._param_slices, model.parameters()) if p.grad is not None and not dead]
    max_norm = 0.5 * FC.live_norm64(eng.grads(), live0) if clip else None
    opt = FusedAdam(model, max_grad_norm=max_norm, skip_nonfinite=clip, ema_decay=0.99 if ema else None, groups=groups,
                    layer_adaptation=True, max_trust_ratio=max_trust, **BASE)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5) if scheduler else None
    names = [k for k, _ in model.named_parameters()]
    fz = FC.frozen_mask(model)
    p_start = bits(eng.flat_params)
    want_tags = (["grad_sumsq_live" if freeze else "grad_sumsq", "grad_norm_finalize"] if clip else []) + \
        ["lamb_moments", "lamb_ratios", "lamb_apply"]
    table_ptr = None
    for step in range(1, steps + 1):
        if accum:
            half = xd.size(0) // 2
            for i, (a, b) in enumerate(((0, half), (half, xd.size(0)))):
                model.loss_and_backward(xd[a:b].contiguous(), hd[a:b].contiguous(), td[a:b].contiguous(), grad_scale=0.5, micro_step=(i, 2))
        else:
            model.loss_and_backward(xd, hd, td)
        m, v = opt._buffers()
        before = [eng.flat_params.detach().cpu().numpy().copy(), eng.grads().cpu().numpy().copy(), m.cpu().numpy().copy(),
                  v.cpu().numpy().copy(), opt.ema.cpu().numpy().copy() if ema else None]
        vals = [(g["lr"], g["eps"], g["weight_decay"], g.get("decoupled_weight_decay", False)) for g in opt.param_groups]
        # the tensors of this step, in named_parameters() order: live, with a gradient
        rows = [(off, off + n, gi, int(_adapts(opt, k, shape, gi)), k) for (k, p), gi, (off, n, shape, dead)
                in zip(model.named_parameters(), opt._group_of, model._param_slices) if p.grad is not None and not dead]
        gn_ref = torch.stack([p.grad.double().norm().cpu() for p, (off, n, shape, dead) in zip(model.parameters(), model._param_slices)
                              if p.grad is not None and not dead])
        gn = opt.grad_norms()
        assert opt.tensor_names == [r[4] for r in rows] and opt.tensor_adapts == [bool(r[3]) for r in rows]
        assert gn.dtype == torch.float64 and float(((gn.cpu() - gn_ref).abs() / gn_ref).max()) <= SUMSQ_TOL
        tags = PC.launch_sequence(lib, opt.step)
        assert tags == want_tags, tags
        if table_ptr is None:
            table_ptr = opt._lamb[1]["table"].table.data_ptr()
        assert opt._lamb[1]["table"].table.data_ptr() == table_ptr   # the device table is built once
        coef = 1.0
        if clip:
            norm = FC.live_norm64(torch.from_numpy(before[1]), [(r[0], r[1]) for r in rows])
            coef = min(1.0, max_norm / (norm + 1e-6))
            assert coef < 1.0 or step > 1
        quads = [r[:4] for r in rows]
        ref = ref_step(*before[:4], before[4], quads, vals, step, coef=coef, max_trust=max_trust, w=ema_weight(0.99, True, step))
        got = [eng.flat_params.detach().cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), opt.ema.cpu().numpy() if ema else None]
        stats = torch.stack([opt.weight_norms, opt.update_norms, opt.trust_ratios], dim=1).cpu().numpy().astype(np.float64)
        assert_step((step,), quads, vals, got, ref[:4], stats, ref[4])
        assert any(r[3] for r in rows) and not all(r[3] for r in rows)
        if sched is not None:
            sched.step()
            assert all(g["lr"] < g["initial_lr"] for g in opt.param_groups)
    assert opt.steps_applied() == steps
    assert torch.equal(bits(eng.flat_params)[fz], p_start[fz])
    assert not torch.equal(bits(eng.flat_params)[~fz], p_start[~fz])
    assert len(names) >= len(opt.tensor_names)
    if freeze:
        assert len(names) > len(opt.tensor_names) + 2


def check_default_adaptation_by_shape(lib, dev):
    """Biases follow Adam's bits and matrices adapt; a group key overrides it both ways."""
    def run(**kw):
        cfg, model, _, (xd, hd, td) = FC.tiny_model(lib, dev)
        opt = FusedAdam(model, **dict(BASE, **kw))
        model.loss_and_backward(xd, hd, td)
        opt.step()
        return model, opt

    adam_model, _ = run(groups=[(r"bias$", {})])   # (the grouped Adam launch: the same grouping, no adaptation)
    model, opt = run(layer_adaptation=True, groups=[(r"bias$", {})])
    ratios = dict(zip(opt.tensor_names, opt.trust_ratios.cpu().tolist()))
    norms = dict(zip(opt.tensor_names, opt.weight_norms.cpu().tolist()))
    flipped, fopt = run(layer_adaptation=True, groups=[(r"bias$", {"layer_adaptation": True}), (r"weight$", {"layer_adaptation": False})])
    fnorms = dict(zip(fopt.tensor_names, fopt.weight_norms.cpu().tolist()))
    fratios = dict(zip(fopt.tensor_names, fopt.trust_ratios.cpu().tolist()))
    seen = set()
    for (k, p), (off, n, shape, dead) in zip(model.named_parameters(), model._param_slices):
        if dead:
            continue
        a, b, c = (bits(mdl.engine.flat_params)[off:off + n] for mdl in (model, adam_model, flipped))
        if len(shape) == 1:
            assert torch.equal(a, b) and ratios[k] == 1.0 and norms[k] == 0.0, k
            assert not torch.equal(c, b) and fnorms[k] > 0.0, k
        else:
            assert not torch.equal(a, b) and norms[k] > 0.0 and ratios[k] != 1.0, k
            assert torch.equal(c, b) and fratios[k] == 1.0 and fnorms[k] == 0.0, k
        seen.add(len(shape) == 1)
    assert seen == {True, False}


def check_off_is_todays_optimizer(lib, dev):
    """layer_adaptation=False: the launches, the bits and the checkpoint keys of an optimizer built without the keyword."""
    for kw, tags in ((dict(), ["adam"]), (dict(max_grad_norm=0.05, skip_nonfinite=True, ema_decay=0.99),
                                          ["grad_sumsq", "grad_norm_finalize", "adam_guarded_ema"]),
                     (dict(groups=GC.GROUPS), ["adam_groups"])):
        runs = []
        for extra in (dict(), dict(layer_adaptation=False, max_trust_ratio=None)):
            cfg, model, _, (xd, hd, td) = FC.tiny_model(lib, dev)
            opt = FusedAdam(model, **dict(BASE, **dict(kw, **extra)))
            for _ in range(2):
                model.loss_and_backward(xd, hd, td)
                assert PC.launch_sequence(lib, opt.step) == tags
            runs.append((bits(model.engine.flat_params), opt.state_dict()))
        assert torch.equal(runs[0][0], runs[1][0])
        a, b = runs[0][1], runs[1][1]
        assert list(a["state"].keys()) == list(b["state"].keys())
        assert [sorted(g.keys()) for g in a["param_groups"]] == [sorted(g.keys()) for g in b["param_groups"]]
        assert not any("layer_adaptation" in g or "max_trust_ratio" in g for g in b["param_groups"])
        for key in a["state"]:
            assert all(torch.equal(a["state"][key][f], b["state"][key][f]) for f in ("step", "exp_avg", "exp_avg_sq"))


def check_checkpoint(lib, dev):
    """A LAMB checkpoint is in torch.optim.Adam's format: it loads into a plain FusedAdam and into torch.optim.Adam, and back."""
    cfg, model, _, (xd, hd, td) = FC.tiny_model(lib, dev)
    opt = FusedAdam(model, layer_adaptation=True, **BASE)
    for _ in range(2):
        model.loss_and_backward(xd, hd, td)
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd.keys()) == ["param_groups", "state"] and len(sd["param_groups"]) == 1
    assert all(sorted(st.keys()) == ["exp_avg", "exp_avg_sq", "step"] for st in sd["state"].values())
    m, v = opt._buffers()
    topt = torch.optim.Adam(list(model.parameters()), lr=1.0)
    topt.load_state_dict(sd)
    for p, (off, n, shape, dead) in zip(model.parameters(), model._param_slices):
        if not dead:
            assert torch.equal(topt.state[p]["exp_avg"].cpu(), m[off:off + n].view(shape).cpu())
    assert topt.param_groups[0]["lr"] == BASE["lr"]

    def resumed(**kw):
        mdl = WaveNet(*TINY, _library=lib)
        mdl.load_state_dict(model.state_dict())
        mdl.to(dev)
        return mdl, FusedAdam(mdl, **kw)

    plain_model, plain = resumed(lr=9.0)                         # ... into a plain FusedAdam (through torch's copy of it)
    plain.load_state_dict(topt.state_dict())
    assert plain.steps_applied() == 2 and plain.param_groups[0]["lr"] == BASE["lr"]
    for a, b in zip(plain._buffers(), opt._buffers()):
        assert torch.equal(bits(a), bits(b))
    plain_model.loss_and_backward(xd, hd, td)
    assert PC.launch_sequence(lib, plain.step) == ["adam"]
    back_model, back = resumed(layer_adaptation=True, lr=9.0)    # ... and back: the resumed LAMB run continues bit for bit
    back.load_state_dict(sd)
    for mdl, o in ((model, opt), (back_model, back)):
        mdl.loss_and_backward(xd, hd, td)
        o.step()
    assert torch.equal(bits(model.engine.flat_params), bits(back_model.engine.flat_params))
    assert torch.equal(bits(opt.trust_ratios), bits(back.trust_ratios))
    for a, b in zip(opt._buffers(), back._buffers()):
        assert torch.equal(bits(a), bits(b))


def check_changed_set_rebuilds_the_table_once(lib, dev):
    cfg, model, _, (xd, hd, td) = FC.tiny_model(lib, dev)
    opt = FusedAdam(model, layer_adaptation=True, **BASE)
    model.loss_and_backward(xd, hd, td)
    opt.step()
    first, n_all = opt._lamb[1]["table"], len(opt.tensor_names)
    model.loss_and_backward(xd, hd, td)
    opt.step()
    assert opt._lamb[1]["table"] is first
    assert model.freeze(r"\.1\.") > 0
    frozen = bits(model.engine.flat_params)
    for _ in range(2):
        model.loss_and_backward(xd, hd, td)
        opt.step()
        second = opt._lamb[1]["table"]
        assert second is not first and len(opt.tensor_names) < n_all and opt.trust_ratios.numel() == len(opt.tensor_names)
    assert opt._lamb[1]["table"] is second
    fz = FC.frozen_mask(model)
    assert torch.equal(bits(model.engine.flat_params)[fz], frozen[fz])
    for p in model.parameters():   # an empty live set launches nothing and counts no step
        p.grad = None
    assert PC.launch_sequence(lib, opt.step) == [] and opt.steps_applied() == 4


def check_constructor(lib, dev):
    cfg, model, _, _ = FC.tiny_model(lib, dev)
    for kw, text in ((dict(layer_adaptation=True, max_trust_ratio=0.0), "max_trust_ratio"),
                     (dict(layer_adaptation=True, max_trust_ratio=-1.0), "max_trust_ratio"),
                     (dict(max_trust_ratio=2.0), "layer_adaptation=True"),
                     (dict(layer_adaptation=True, groups=[(r"bias$", {"layer_adaptation": 1})]), "True or False"),
                     (dict(layer_adaptation=True, groups=[(r"bias$", {"layer_adaptation": "false"})]), "True or False"),
                     (dict(groups=[(r"bias$", {"layer_adaptation": True})]), "layer_adaptation=False"),
                     (dict(layer_adaptation=True, groups=[(r"bias$", {"trust": 1.0})]), "unknown key")):
        try:
            FusedAdam(model, **kw)
        except ValueError as err:
            assert text in str(err), (text, str(err))
        else:
            raise AssertionError("FusedAdam(%r) must raise" % (kw,))
    opt = FusedAdam(model, layer_adaptation=True, max_trust_ratio=10.0, groups=[(r"bias$", {"layer_adaptation": True})])
    assert opt.max_trust_ratio == 10.0 and opt.param_groups[1]["layer_adaptation"] is True
    assert "layer_adaptation" not in opt.param_groups[0]
    try:
        opt.trust_ratios
    except RuntimeError as err:
        assert "no step() yet" in str(err)
    else:
        raise AssertionError("trust_ratios before the first step must raise")
    try:
        FusedAdam(model).trust_ratios
    except RuntimeError as err:
        assert "layer_adaptation=False" in str(err)
    else:
        raise AssertionError("trust_ratios without layer adaptation must raise")
