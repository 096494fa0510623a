# -*- coding: utf-8 -*-
"""Parameter groups in FusedAdam (wn_group_table / wn_adam_step_groups / wn_grad_norm_groups /
wn_adam_step_guarded_groups, ``FusedAdam(groups=)``): the cases tests/test_emu_groups.py runs on the host-compiled kernels and
tests/test_gpu_groups.py on the MI355X.

References: numpy, torch on the CPU (``torch.optim.Adam`` with param groups, ``decoupled_weight_decay`` per group = AdamW), the
oracle's gradients, or the library's own single-group entry points where the claim IS bit-identity with them.  Tolerances are the
project's: ``PC.TOL_ADAM_REL_LR`` x the group's lr for weights (tests/parity_common.py), ``CC.MOMENT_TOL`` of the maximum for moments
(tests/clip_common.py).
"""
import ctypes
import re

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import clip_common as CC
from tests import freeze_common as FC
from tests import parity_common as PC
from tests.golden_util import GoldenCase

TINY = CC.TINY
LR = 1e-3
BETAS = (0.9, 0.999)
# three groups that differ in all three values: (lr, eps, weight_decay, decoupled)
G3 = [(LR, 1e-8, 0.0, 0), (0.1 * LR, 1e-6, 1e-2, 0), (10.0 * LR, 1e-3, 1e-1, 0)]
G16 = [(LR * (1.0 + 0.25 * i), 1e-8 * 10.0 ** (i % 5), 1e-3 * i, 0) for i in range(16)]
bits = FC.bits


def group_array(vals):
    arr = (_lib.WnAdamGroup * len(vals))()
    for a, (lr, eps, wd, dec) in zip(arr, vals):
        a.lr, a.eps, a.weight_decay, a.decoupled = lr, eps, wd, int(dec)
    return arr


def make_group_table(lib, dev, ranges, gids, n, n_groups):
    """(device table, n_ranges, n_live) through wn_group_table, its words checked against a numpy restatement and against
    wn_live_table on the same ranges."""
    nr = len(ranges)
    flat = (ctypes.c_int64 * (3 * nr))(*[x for (lo, hi), g in zip(ranges, gids) for x in (lo, hi, g)])
    host = torch.zeros(4 * nr, dtype=torch.int64)
    n_live = lib.wn_group_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, n_groups, ctypes.c_void_p(host.data_ptr()))
    assert n_live == sum(hi - lo for lo, hi in ranges), lib.wn_last_error()
    lo, hi = np.array([r[0] for r in ranges]), np.array([r[1] for r in ranges])
    want = np.concatenate([lo, hi, np.cumsum(hi - lo) - (hi - lo), np.array(gids)])
    assert np.array_equal(host.numpy(), want)
    live, nr2, n_live2 = FC.make_table(lib, "cpu", ranges, n)
    assert nr2 == nr and n_live2 == n_live and torch.equal(host[:3 * nr], live)
    return host.to(dev), nr, int(n_live)


def check_group_table(lib):
    make_group_table(lib, "cpu", [(0, 10), (10, 20), (50, 100)], [2, 0, 2], 100, 3)   # touching ranges, a group without a range
    make_group_table(lib, "cpu", [(i, i + 1) for i in range(0, 64, 2)], [i % 16 for i in range(32)], 64, 16)

    def error(triples, n=100, n_groups=3, null=None):
        nr = len(triples)
        flat = (ctypes.c_int64 * max(3 * nr, 1))(*[x for t in triples for x in t])
        host = torch.zeros(max(4 * nr, 1), dtype=torch.int64)
        rc = lib.wn_group_table(None if null == "triples" else ctypes.cast(flat, ctypes.c_void_p), nr, n, n_groups,
                                None if null == "table" else ctypes.c_void_p(host.data_ptr()))
        msg = lib.wn_last_error().decode()
        assert rc == -1 and "wn_group_table" in msg, (triples, rc, msg)
        return msg

    assert "NULL" in error([(0, 4, 0)], null="triples") and "NULL" in error([(0, 4, 0)], null="table")
    assert "empty table" in error([])
    assert "n <= 0" in error([(0, 4, 0)], n=0)
    assert "sorted and disjoint" in error([(10, 20, 0), (0, 5, 0)]) and "sorted and disjoint" in error([(0, 10, 0), (9, 20, 1)])
    assert "outside" in error([(0, 10, 0), (90, 101, 0)]) and "outside" in error([(-1, 10, 0)])
    assert "is empty" in error([(5, 5, 0)]) and "is empty" in error([(7, 3, 0)])
    assert "group" in error([(0, 4, 3)]) and "group" in error([(0, 4, -1)])
    assert "n_groups" in error([(0, 4, 0)], n_groups=0) and "n_groups" in error([(0, 4, 0)], n_groups=17)


# ---- op level: the three entry points ------------------------------------------------------------------------------------------
def new_block(dev):
    return torch.zeros(_lib.MAX_PARAM_GROUPS * 4, dtype=torch.float32, device=dev)


def run_norm_groups(lib, dev, g, table, vals, max_norm=0.0, guard=False, state=None, scratch=None, block=None, whole_skip=None,
                    betas=BETAS):
    """wn_grad_norm_groups; ``whole_skip=(lo, hi)``: the whole-buffer sum of squares (table NULL) without that range."""
    tab, nr, n_live = table
    state = CC.new_state(dev) if state is None else state
    scratch = CC.new_scratch(lib, g.numel(), dev) if scratch is None else scratch
    block = new_block(dev) if block is None else block
    arr = group_array(vals)
    lo, hi = (0, 0) if whole_skip is None else whole_skip
    lib.check(lib.wn_grad_norm_groups(_ptr(g), g.numel(), None if whole_skip is not None else _ptr(tab), nr, n_live, lo, hi,
                                      float(max_norm), int(guard), ctypes.cast(arr, ctypes.c_void_p), len(vals), betas[0], betas[1],
                                      _ptr(scratch), _ptr(state), _ptr(block), _stream_handle(torch.device(dev))),
              "wn_grad_norm_groups")
    return state, block


def adam_groups(lib, dev, variant, p, g, m, v, e, table, vals, state, block, step, decay=0.999, warm=1, betas=BETAS):
    n, st = p.numel(), _stream_handle(torch.device(dev))
    tab, nr, n_live = table
    ema = _ptr(e) if "ema" in variant else None
    if variant in ("plain", "ema"):
        arr = group_array(vals)
        rc = lib.wn_adam_step_groups(_ptr(p), _ptr(g), _ptr(m), _ptr(v), ema, n, _ptr(tab), nr, n_live, step,
                                     ctypes.cast(arr, ctypes.c_void_p), len(vals), betas[0], betas[1], decay, warm, st)
    else:
        rc = lib.wn_adam_step_guarded_groups(_ptr(p), _ptr(g), _ptr(m), _ptr(v), ema, n, _ptr(tab), nr, n_live, _ptr(block),
                                             _ptr(state), decay, warm, st)
    lib.check(rc, "groups " + variant)


def layouts(n):
    """(name, ranges, group ids, group values): the range lists of tests/freeze_common.py with round-robin ids over three groups,
    and at n = 1023 one layout of 16 groups and one where a group owns no range."""
    out = []
    for name, ranges in FC.tables(n):
        if n == CC.N_BIG and name not in FC.BIG_TABLES:
            continue
        out.append((name, ranges, [i % 3 for i in range(len(ranges))], G3))
    if n == 1023:
        cuts = list(range(0, n, 21)) + [n]
        r40 = [(a + (i % 2), b) for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]   # touching and separated neighbours
        out.append(("16_groups", r40, [i % 16 for i in range(len(r40))], G16))
        out.append(("a_group_without_a_range", r40, [0 if i % 2 else 2 for i in range(len(r40))], G3))
    return out


def check_adam_groups(lib, dev, n, misalign, only=None):
    """For each variant of FC.VARIANTS: the grouped entry point against the stitched results of the ``_live`` entry point, run per
    group on copies with that group's ranges and scalars (the guarded ones with a state block made with lr = lr_g).  p, m, v, e
    bit-equal on every live element and bit-equal to the inputs outside (g, m, v hold NaN there); g is never written."""
    step, decay, warm = 3, 0.999, 1
    rs = np.random.RandomState(29 + n)
    mk = lambda a: FC._misaligned(torch.from_numpy(np.asarray(a, np.float32)), misalign, dev)   # noqa: E731
    for name, ranges, gids, vals in layouts(n):
        if only is not None and name not in only:
            continue
        what = (n, misalign, name)
        table = make_group_table(lib, dev, ranges, gids, n, len(vals))
        live = FC.live_mask(n, ranges)
        dead = ~live
        p0, e0 = mk(rs.standard_normal(n)), mk(rs.standard_normal(n))
        g0, m0, v0 = mk(rs.standard_normal(n)), mk(0.1 * rs.standard_normal(n)), mk(0.01 * rs.uniform(size=n))
        for buf in (g0, m0, v0):
            buf[dead.to(dev)] = float("nan")
        max_norm = 0.5 * FC.live_norm64(g0, ranges)

        def norm(vals_):
            state = CC.new_state(dev)
            state[3] = step - 1
            return run_norm_groups(lib, dev, g0, table, vals_, max_norm=max_norm, guard=True, state=state)

        state, block = norm(vals)
        st = CC.read_state(state)
        assert st.apply == 1 and st.steps_applied == step and st.clip_coef < 1.0
        used = sorted(set(gids))
        for variant in FC.VARIANTS:
            fresh = lambda: [FC._misaligned(x.cpu(), misalign, dev) for x in (p0, g0, m0, v0, e0)]   # noqa: E731
            a = fresh()
            adam_groups(lib, dev, variant, *a, table, vals, state, block, step, decay, warm)
            want = [bits(x) for x in (p0, g0, m0, v0, e0)]
            for gi in used:
                mine = [r for r, g_ in zip(ranges, gids) if g_ == gi]
                lr, eps, wd, _ = vals[gi]
                sub = FC.make_table(lib, dev, mine, n)
                gstate = CC.new_state(dev)   # the single-group state block: the norm over ALL live ranges, lr = lr_g
                gstate[3] = step - 1
                FC.run_norm_live(lib, dev, g0, table, max_norm=max_norm, guard=True, state=gstate, lr=lr, betas=BETAS)
                b = fresh()
                FC._adam_live(lib, dev, variant, *b, sub, gstate, step, (lr, BETAS[0], BETAS[1], eps, wd, decay, warm))
                mask = FC.live_mask(n, mine)
                for w, y in zip(want, b):
                    w[mask] = bits(y)[mask]
            for x, w, x0, name_ in zip(a, want, (p0, g0, m0, v0, e0), "pgmve"):
                assert torch.equal(bits(x)[live], w[live]), what + (variant, name_, "live elements")
                assert torch.equal(bits(x)[dead], bits(x0)[dead]), what + (variant, name_, "outside the ranges")
            assert torch.equal(bits(a[1]), bits(g0)), what + (variant, "g written")
            assert not torch.equal(bits(a[0])[live], bits(p0)[live])
            assert torch.equal(bits(a[4]), bits(e0)) == ("ema" not in variant)
            if len(used) > 1:   # not vacuous: every range with group 0's scalars gives other bits
                same = [vals[0]] * len(vals)
                sstate, sblock = norm(same)
                c = fresh()
                adam_groups(lib, dev, variant, *c, table, same, sstate, sblock, step, decay, warm)
                assert not torch.equal(bits(c[0])[live], want[0][live]) and not torch.equal(bits(c[2])[live], want[2][live]), \
                    what + (variant, "vacuous")


def check_guarded_scalars(lib, dev, misalign=1):
    n = 4097
    ranges = [(3, 1021), (1022, 1023), (2055, 4090)]
    gids = [0, 1, 2]
    table = make_group_table(lib, dev, ranges, gids, n, 3)
    g = CC.buffer(n, misalign, dev)
    max_norm = 0.5 * FC.live_norm64(g, ranges)

    def start(dev_):
        s = CC.new_state(dev_)
        s[3] = 4
        return s

    state, block = run_norm_groups(lib, dev, g, table, G3, max_norm=max_norm, guard=True, state=start(dev))
    first = (CC.state_bits(state), bits(block).tolist())
    # the state block: wn_grad_norm_live's with lr = lr_0; each group's lr / bc1: the state block's of a run with lr = lr_g
    for gi, (lr, eps, wd, _) in enumerate(G3):
        ref = FC.run_norm_live(lib, dev, g, table, max_norm=max_norm, guard=True, state=start(dev), lr=lr, betas=BETAS)
        if gi == 0:
            assert torch.equal(state.cpu(), ref.cpu()), "state block"
        w = block.cpu().view(torch.int32)[4 * gi:4 * gi + 4]
        assert int(w[0]) == int(ref.cpu().view(torch.int32)[10]), ("lr / bc1", gi)
        assert torch.equal(w[1:], torch.tensor([eps, wd, 1.0], dtype=torch.float32).view(torch.int32)), gi
    assert not bool(block[12:].any())   # zeros behind n_groups
    # nothing frozen: the whole-buffer sum of squares with the skip range, wn_grad_norm's state block
    whole = make_group_table(lib, dev, [(0, 1021), (1021, 2000), (2055, n)], gids, n, 3)
    s2, b2 = run_norm_groups(lib, dev, g, whole, G3, max_norm=max_norm, guard=True, state=start(dev), whole_skip=(2000, 2055))
    ref = CC.run_norm(lib, dev, g, 2000, 2055, max_norm=max_norm, guard=True, state=start(dev), lr=G3[0][0], betas=BETAS)
    assert torch.equal(s2.cpu(), ref.cpu())
    # a poisoned state, scratch or group block changes no bit
    s3, scratch, b3 = start(dev), CC.new_scratch(lib, n, dev), new_block(dev)
    CC.poison(s3, scratch)
    b3.fill_(float("nan"))
    run_norm_groups(lib, dev, g, table, G3, max_norm=max_norm, guard=True, state=s3, scratch=scratch, block=b3)
    assert (CC.state_bits(s3), bits(b3).tolist()) == first
    # a NaN in a live element of any group: apply = 0, lr / bc1 = 0 everywhere, and the Adam launch writes nothing in any group
    rs = np.random.RandomState(5)
    for idx in (3, 1022, 4089):
        gb = CC.buffer(n, misalign, dev)
        gb[idx] = float("nan")
        s4, b4 = run_norm_groups(lib, dev, gb, table, G3, max_norm=max_norm, guard=True, state=start(dev))
        st = CC.read_state(s4)
        assert st.apply == 0 and st.steps_skipped == 1 and st.steps_applied == 4
        assert not bool(b4.view(4 * _lib.MAX_PARAM_GROUPS)[0::4].any())
        for variant in ("guarded", "guarded_ema"):
            bufs = [FC._misaligned(torch.from_numpy(rs.standard_normal(n).astype(np.float32)), misalign, dev) for _ in range(5)]
            bufs[1] = gb
            before = [bits(x) for x in bufs]
            adam_groups(lib, dev, variant, *bufs, table, G3, s4, b4, 5)
            assert all(torch.equal(bits(x), x0) for x, x0 in zip(bufs, before)), (idx, variant)


def check_group_call_errors(lib, dev):
    n = 100
    table = make_group_table(lib, dev, [(0, 10), (10, 20), (50, 100)], [0, 1, 0], n, 2)
    tab, nr, n_live = table
    p, g, m, v, e = (torch.zeros(n, device=dev) for _ in range(5))
    state, scratch, block = CC.new_state(dev), CC.new_scratch(lib, n, dev), new_block(dev)
    st = _stream_handle(torch.device(dev))
    arr = group_array(G3[:2])
    ap = ctypes.cast(arr, ctypes.c_void_p)

    def norm(tab_=tab, nl=n_live, groups=ap, ng=2, block_=block, skip=(0, 0), state_=state):
        return lib.wn_grad_norm_groups(_ptr(g), n, None if tab_ is None else _ptr(tab_), nr, nl, skip[0], skip[1], 0.0, 1, groups, ng,
                                       0.9, 0.999, _ptr(scratch), _ptr(state_), _ptr(block_), st)

    def adam(tab_=tab, nl=n_live, groups=ap, ng=2, step=1, e_=None, decay=0.9):
        return lib.wn_adam_step_groups(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e_), n, _ptr(tab_), nr, nl, step, groups, ng, 0.9, 0.999,
                                       decay, 1, st)

    def guarded(tab_=tab, nl=n_live, block_=block, state_=state, e_=None, decay=0.9):
        return lib.wn_adam_step_guarded_groups(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e_), n, _ptr(tab_), nr, nl, _ptr(block_),
                                               _ptr(state_), decay, 1, st)

    assert norm() == 0 and norm(tab_=None, skip=(20, 50)) == 0 and adam() == 0 and guarded() == 0 and adam(e_=e) == 0 and guarded(e_=e) == 0

    def fails(rc, text):
        assert rc != 0 and text in lib.wn_last_error().decode(), (rc, text, lib.wn_last_error())

    for call, name in ((norm, "wn_grad_norm_groups"), (adam, "wn_adam_step_groups"), (guarded, "wn_adam_step_guarded_groups")):
        fails(call(nl=0), name)
        fails(call(nl=n + 1), name)
    for call in (norm, adam):
        fails(call(groups=None), "groups is NULL")
        fails(call(ng=0), "n_groups")
        fails(call(ng=17), "n_groups")
    fails(norm(block_=None), "group_scalars is NULL")
    fails(guarded(block_=None), "group_scalars is NULL")
    fails(norm(skip=(20, 50)), "skip range")
    fails(norm(tab_=None, skip=(50, 101)), "skip range")
    fails(norm(state_=None), "wn_grad_norm_groups")
    fails(adam(tab_=None), "table is NULL")
    fails(adam(step=0), "wn_adam_step_groups")
    fails(adam(e_=p), "overlaps")
    fails(guarded(state_=None), "wn_adam_step_guarded_groups")
    fails(guarded(e_=e, decay=1.0), "ema_decay")
    eng = WaveNetEngine(*TINY, device=dev, library=lib)
    for bad, ng in (([], 2), ([(0, 5, 2)], 2), ([(0, 5, 0)], 17), ([(10, 20, 0), (0, 5, 0)], 2)):
        try:
            eng.group_table(bad, ng)
        except _lib.WnError as err:
            assert "wn_group_table" in str(err)
        else:
            raise AssertionError("group_table(%r) did not raise" % (bad,))


# ---- decoupled groups against torch ----------------------------------------------------------------------------------------------
def check_decoupled(lib, dev, guarded):
    """Three steps, one torch optimizer with param groups: torch.optim.Adam semantics for the L2 ranges, AdamW's
    (decoupled_weight_decay) for the decoupled ones.  Guarded: the clip active in every step."""
    n = 5003
    ranges = [(0, 1021), (1021, 1290), (1300, 2500), (2501, 4000), (4000, n)]
    gids = [0, 1, 2, 1, 3]
    vals = [(LR, 1e-8, 1e-2, 0), (3 * LR, 1e-8, 1e-1, 1), (0.3 * LR, 1e-6, 1e-2, 1), (LR, 1e-8, 0.0, 1)]
    table = make_group_table(lib, dev, ranges, gids, n, len(vals))
    rs = np.random.RandomState(13)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))   # noqa: E731
    p0, m0, v0 = f32(rs.standard_normal(n)), f32(0.1 * rs.standard_normal(n)), f32(0.01 * rs.uniform(size=n))
    qs = [torch.nn.Parameter(p0[lo:hi].clone()) for lo, hi in ranges]
    l2qs = [torch.nn.Parameter(p0[lo:hi].clone()) for lo, hi in ranges]   # the same groups, every one L2: NOT the reference

    def torch_adam(params, decoupled):
        opt = torch.optim.Adam([{"params": [q for q, g_ in zip(params, gids) if g_ == gi], "lr": lr, "eps": eps, "weight_decay": wd,
                                 "decoupled_weight_decay": bool(dec) and decoupled} for gi, (lr, eps, wd, dec) in enumerate(vals)],
                               betas=BETAS)
        for q, (lo, hi) in zip(params, ranges):
            opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0[lo:hi].clone(), "exp_avg_sq": v0[lo:hi].clone()}
        return opt

    ropt, l2opt = torch_adam(qs, True), torch_adam(l2qs, False)
    p, m, v = p0.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
    state = CC.new_state(dev)
    live = FC.live_mask(n, ranges)
    for step in range(3):
        g0 = f32(rs.standard_normal(n) * (1.0 + step))
        for q, q2, (lo, hi) in zip(qs, l2qs, ranges):
            q.grad = g0[lo:hi].clone()
            q2.grad = g0[lo:hi].clone()
        g = g0.clone().to(dev)
        if guarded:
            max_norm = 0.5 * FC.live_norm64(g0, ranges)
            torch.nn.utils.clip_grad_norm_(qs, max_norm)
            torch.nn.utils.clip_grad_norm_(l2qs, max_norm)
            _, block = run_norm_groups(lib, dev, g, table, vals, max_norm=max_norm, guard=True, state=state)
            st = CC.read_state(state)
            assert st.apply == 1 and st.steps_applied == step + 1 and st.clip_coef < 1.0
            adam_groups(lib, dev, "guarded", p, g, m, v, None, table, vals, state, block, step + 1)
        else:
            adam_groups(lib, dev, "plain", p, g, m, v, None, table, vals, None, None, step + 1)
        ropt.step()
        l2opt.step()
        assert torch.equal(g.cpu(), g0)
        for q, (lo, hi), gi in zip(qs, ranges, gids):
            rst = ropt.state[q]
            e = float((p.cpu()[lo:hi] - q.detach()).abs().max())
            assert e <= PC.TOL_ADAM_REL_LR * vals[gi][0], (step, gi, e)
            for ours, theirs in ((m, rst["exp_avg"]), (v, rst["exp_avg_sq"])):
                assert float((ours.cpu()[lo:hi] - theirs).abs().max()) <= CC.MOMENT_TOL * float(theirs.abs().max()), (step, gi)
        for ours, start in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(bits(ours)[~live], bits(start)[~live])
    # the gate tells the two decay modes apart: the same groups as L2 groups end outside it (groups 1 and 2; group 3 has no decay)
    for q2, (lo, hi), gi in zip(l2qs, ranges, gids):
        assert (float((p.cpu()[lo:hi] - q2.detach()).abs().max()) > PC.TOL_ADAM_REL_LR * vals[gi][0]) == (gi in (1, 2)), gi


def check_decoupled_zero_decay_is_l2_zero_decay(lib, dev):
    n, step = 1023, 2
    ranges = [(1, 500), (502, 1020)]
    rs = np.random.RandomState(3)
    src = [torch.from_numpy(rs.standard_normal(n).astype(np.float32)) for _ in range(5)]
    src[3] = src[3].abs() * 0.01
    out = []
    for dec in (0, 1):
        vals = [(LR, 1e-8, 0.0, dec), (3 * LR, 1e-6, 0.0, dec)]
        table = make_group_table(lib, dev, ranges, [0, 1], n, 2)
        for variant in FC.VARIANTS:
            bufs = [x.clone().to(dev) for x in src]
            state = CC.new_state(dev)
            state[3] = step - 1
            state, block = run_norm_groups(lib, dev, bufs[1], table, vals, max_norm=1.0, guard=True, state=state)
            adam_groups(lib, dev, variant, *bufs, table, vals, state, block, step)
            out.append([bits(x) for x in bufs])
    half = len(out) // 2
    for a, b in zip(out[:half], out[half:]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(out[0][0], bits(src[0]))


# ---- module level ------------------------------------------------------------------------------------------------------------------
GROUPS = [(r"bias$", {"lr": 3e-3, "weight_decay": 0.0}),
          (r"^conv_post|skip_1x1", {"lr": 1e-4, "weight_decay": 0.1, "decoupled_weight_decay": True, "eps": 1e-6})]
BASE = dict(lr=1e-3, weight_decay=1e-2, eps=1e-8)


def torch_groups(named, groups=GROUPS, base=BASE):
    """The param-group dicts torch.optim.Adam takes for ``(key, Parameter)`` pairs: restated here, first matching entry wins."""
    out = [dict(base, params=[], decoupled_weight_decay=False)]
    for _, values in groups:
        out.append(dict(dict(base, decoupled_weight_decay=False), **values))
        out[-1]["params"] = []
    index = {}
    for k, p in named:
        gi = next((1 + j for j, (rx, _) in enumerate(groups) if re.search(rx, k)), 0)
        out[gi]["params"].append(p)
        index[k] = gi
    return out, index


def _model(lib, dev, case):
    if case is None:
        cfg, model, (x, h, t), dbatch = FC.tiny_model(lib, dev)
        return cfg, model, (x, h, t), dbatch, 3
    g = GoldenCase(case)
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(dev)
    return g.cfg, model, (g.x, g.h, g.t), (g.x.to(dev), g.h.to(dev), g.t.to(dev)), g.adam_steps


def check_module(lib, dev, case=None, clip=False, ema=False, freeze=None, scheduler=False):
    """FusedAdam(groups=) against torch.optim.Adam with the same groups on the oracle's gradients."""
    cfg, model, (x, h, t), (xd, hd, td), steps = _model(lib, dev, case)
    if freeze:
        assert model.freeze(freeze) > 0
    frozen = {k for k, p in model.named_parameters() if not p.requires_grad}
    ref = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    _, _, og = O.train_step(cfg, {k: v.detach() for k, v in ref.items()}, None, x, h, t)
    trainable = [k for k in ref if k not in frozen and og[k] is not None]
    tgroups, index = torch_groups([(k, ref[k]) for k in trainable])
    assert all(len(g["params"]) > 0 for g in tgroups)
    if freeze:   # the freeze set cuts through every group
        assert {index_ for k, index_ in torch_groups([(k, ref[k]) for k in frozen])[1].items()} == {0, 1, 2}
    ropt = torch.optim.Adam(tgroups, betas=BETAS)
    max_norm = None
    if clip:
        max_norm = 0.5 * float(np.sqrt(sum(float((og[k].double() ** 2).sum()) for k in trainable)))
    opt = FusedAdam(model, max_grad_norm=max_norm, skip_nonfinite=clip, ema_decay=0.99 if ema else None, groups=GROUPS, **BASE)
    assert len(opt.param_groups) == 3
    if scheduler:
        steps = 5
        scheds = [torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5) for o in (opt, ropt)]
    eng = model.engine
    p_start = bits(eng.flat_params)
    e_ref = eng.flat_params.detach().cpu().double().clone()
    fz = FC.frozen_mask(model)
    active, ptr = 0, None
    want_tags = (["grad_sumsq_live" if freeze else "grad_sumsq", "grad_norm_finalize"] if clip else []) + \
        ["adam%s%s_groups" % ("_guarded" if clip else "", "_ema" if ema else "")]
    for step in range(steps):
        _, _, og = O.train_step(cfg, {k: v_.detach() for k, v_ in ref.items()}, None, x, h, t)
        for k in trainable:
            ref[k].grad = og[k].clone()
        if clip:
            tnorm = float(torch.nn.utils.clip_grad_norm_([ref[k] for k in trainable], max_norm))
            active += tnorm > max_norm
        ropt.step()
        model.loss_and_backward(xd, hd, td)
        tags = PC.launch_sequence(lib, opt.step)
        assert tags == want_tags, tags   # one Adam launch (three guarded); nothing frozen: the whole-buffer sum of squares
        if ptr is None:
            ptr = opt._route[2].table.data_ptr()
        assert opt._route[2].table.data_ptr() == ptr   # the device table is built once
        if scheduler:
            for s in scheds:
                s.step()
            for g_, tg in zip(opt.param_groups, ropt.param_groups):
                assert g_["lr"] == tg["lr"] and g_["lr"] < tg["initial_lr"]
        if ema:
            d = min(0.99, (1.0 + step + 1) / (10.0 + step + 1))
            e_ref += (1.0 - d) * (eng.flat_params.detach().cpu().double() - e_ref)
    assert opt.steps_applied() == steps
    if clip:
        assert active == steps, "the clip must be active in every step"
    sd = model.state_dict()
    lr0 = [BASE["lr"]] + [v.get("lr", BASE["lr"]) for _, v in GROUPS]
    mc, vc = (b.cpu() for b in opt._buffers())
    for k, (off, n, shape, dead) in zip(sd.keys(), model._param_slices):
        if k not in trainable:
            continue
        e = float((sd[k].cpu() - ref[k].detach()).abs().max())
        assert e <= PC.TOL_ADAM_REL_LR * lr0[index[k]], "%s (group %d): |dw| err %g" % (k, index[k], e)
        rst = ropt.state[ref[k]]
        for ours, theirs in ((mc, rst["exp_avg"]), (vc, rst["exp_avg_sq"])):
            assert float((ours[off:off + n].view(shape) - theirs).abs().max()) <= CC.MOMENT_TOL * float(theirs.abs().max()), k
    assert torch.equal(bits(eng.flat_params)[fz], p_start[fz])
    assert not torch.equal(bits(eng.flat_params)[~fz], p_start[~fz])
    if ema:
        # per step one rounding of w and one of the fma: 2 * 2^-24 of the largest average, over `steps` steps
        got = opt.ema.detach().cpu().double()
        assert float((got - e_ref)[~fz].abs().max()) <= 2 * steps * 2.0 ** -24 * float(e_ref.abs().max())
        assert torch.equal(bits(opt.ema)[fz], p_start[fz])


def check_without_groups_is_todays_optimizer(lib, dev):
    """groups=None: launch tags, result bits and checkpoint keys of a plainly constructed optimizer; one L2 group that holds every
    tensor takes the single-group launch with that group's values."""
    runs = []
    for kw in (dict(groups=None), dict(), dict(groups=[(r".", {"lr": 1e-3, "weight_decay": 1e-2})], lr=7.0, weight_decay=0.5)):
        cfg, model, _, (xd, hd, td) = FC.tiny_model(lib, dev)
        kw.setdefault("lr", 1e-3)
        kw.setdefault("weight_decay", 1e-2)
        opt = FusedAdam(model, **kw)
        for _ in range(2):
            model.loss_and_backward(xd, hd, td)
            assert PC.launch_sequence(lib, opt.step) == ["adam"]
        runs.append((bits(model.engine.flat_params), opt.state_dict()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], runs[2][0])
    a, b = runs[0][1], runs[1][1]
    assert list(a["state"].keys()) == list(b["state"].keys()) and len(a["param_groups"]) == 1
    assert a["param_groups"] == b["param_groups"] and "decoupled_weight_decay" not in a["param_groups"][0]
    assert a["param_groups"][0]["params"] == list(range(len(list(model.parameters()))))


def check_constructor(lib, dev):
    cfg, model, _, _ = FC.tiny_model(lib, dev)
    names = [k for k, _ in model.named_parameters()]
    opt = FusedAdam(model, groups=GROUPS, **BASE)
    assert [len(g["params"]) for g in opt.param_groups] == [sum(1 for k in names if torch_groups([(k, None)])[1][k] == gi) for gi in range(3)]
    assert opt.param_groups[1]["weight_decay"] == 0.0 and opt.param_groups[1]["eps"] == BASE["eps"]          # a missing key inherits
    assert opt.param_groups[2]["decoupled_weight_decay"] is True and opt.param_groups[0]["decoupled_weight_decay"] is False
    assert all(isinstance(p, torch.nn.Parameter) for g in opt.param_groups for p in g["params"])
    for bad, text in (([(r"no_such_tensor", {})], "matches no parameter"), ([(r"bias$", {"betas": (0.5, 0.9)})], "per optimizer"),
                      ([(r"bias$", {"momentum": 0.9})], "unknown key"), ([(r".", {})] * 16, "at most 16")):
        try:
            FusedAdam(model, groups=bad)
        except ValueError as err:
            assert text in str(err), (text, str(err))
        else:
            raise AssertionError("groups=%r must raise" % (bad,))
    FusedAdam(model, groups=[(r".", {})] * 15)
    for o in (opt, FusedAdam(model)):
        try:
            o.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))]})
        except RuntimeError as err:
            assert "fixed at construction" in str(err)
        else:
            raise AssertionError("add_param_group must raise")


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
def check_checkpoint(lib, dev):
    kw = dict(groups=GROUPS, max_grad_norm=0.05, skip_nonfinite=True, **BASE)
    cfg, model, (x, h, t), (xd, hd, td) = FC.tiny_model(lib, dev)
    opt = FusedAdam(model, **kw)
    for _ in range(2):
        model.loss_and_backward(xd, hd, td)
        opt.step()
    sd = opt.state_dict()
    n_tensors = len(model._param_slices)
    lists = [g["params"] for g in sd["param_groups"]]
    assert len(lists) == 3 and sorted(i for lst in lists for i in lst) == list(range(n_tensors))   # tile, no overlap
    assert all(lst == list(range(lst[0], lst[0] + len(lst))) for lst in lists if lst)
    assert len(sd["state"]) == sum(not dead for (_, _, _, dead) in model._param_slices)
    # ... into torch.optim.Adam built with the same groups over the model's parameters, and back
    tgroups, _ = torch_groups(list(model.named_parameters()))
    topt = torch.optim.Adam(tgroups, betas=BETAS)
    topt.load_state_dict(sd)
    named = dict(model.named_parameters())
    m, v = opt._buffers()
    for k, (off, n, shape, dead) in zip(named, model._param_slices):   # torch holds OUR moments under the same tensors
        if not dead:
            assert torch.equal(topt.state[named[k]]["exp_avg"].cpu(), m[off:off + n].view(shape).cpu()), k
    assert [g["lr"] for g in topt.param_groups] == [1e-3, 3e-3, 1e-4] and topt.param_groups[2]["decoupled_weight_decay"] is True
    resumed = WaveNet(*TINY, _library=lib)
    resumed.load_state_dict(model.state_dict())
    resumed.to(dev)
    ropt = FusedAdam(resumed, **dict(kw, lr=9.0, weight_decay=0.7))   # (the checkpoint's values win)
    ropt.load_state_dict(topt.state_dict())
    assert (ropt.steps_applied(), ropt.steps_skipped()) == (2, 0)
    assert [g["lr"] for g in ropt.param_groups] == [1e-3, 3e-3, 1e-4] and ropt.param_groups[0]["weight_decay"] == 1e-2
    # training continues: the resumed optimizer bit for bit, torch (CPU copy of the same state) to the project's gates
    ref = {k: torch.nn.Parameter(p.detach().cpu().clone()) for k, p in named.items()}
    cgroups, index = torch_groups(list(ref.items()))
    copt = torch.optim.Adam(cgroups, betas=BETAS)
    copt.load_state_dict(sd)
    _, _, og = O.train_step(cfg, {k: p.detach() for k, p in ref.items()}, None, x, h, t)
    for k, p in ref.items():
        p.grad = None if og[k] is None else og[k].clone()
    torch.nn.utils.clip_grad_norm_([p for p in ref.values() if p.grad is not None], 0.05)
    copt.step()
    for mdl, o in ((model, opt), (resumed, ropt)):
        mdl.loss_and_backward(xd, hd, td)
        o.step()
    assert torch.equal(bits(model.engine.flat_params), bits(resumed.engine.flat_params))
    for a, b in zip(opt._buffers(), ropt._buffers()):
        assert torch.equal(bits(a), bits(b))
    lr0 = [1e-3, 3e-3, 1e-4]
    for k, w in model.state_dict().items():
        if og[k] is not None:
            assert float((w.cpu() - ref[k].detach()).abs().max()) <= PC.TOL_ADAM_REL_LR * lr0[index[k]], k
    # a different structure raises, as torch does
    for other in (FusedAdam(resumed), FusedAdam(resumed, groups=GROUPS[:1]), FusedAdam(resumed, groups=[GROUPS[0], (r"^conv_post", {})])):
        try:
            other.load_state_dict(sd)
        except ValueError as err:
            assert "parameter group" in str(err)
        else:
            raise AssertionError("a mismatched group structure must raise")
