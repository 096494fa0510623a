# -*- coding: utf-8 -*-
"""Low-rank adapters (wn_lora_table / wn_lora_merge / wn_lora_project, ``LowRankAdapters``, ``AdapterAdam``): the
cases tests/test_emu_lora.py runs on the host-compiled kernels and tests/test_gpu_lora.py on the MI355X.

The reference of every numeric check is the same expression in numpy float64 from the fp32 inputs -- never the code under test.

Tolerances, derived (u = 2^-24, every fp32 operation rounds once, relative error at most u; no product here underflows, magnitudes
stay inside [1e-6, 1e6]):
  project   an element is a sum of n products (n = rows for dA, cols for dB) formed by fma chains inside a tile, the tiles' shares
            added in order, and one multiplication by scale: every product passes through at most n + 1 roundings, so
            |err| <= ((1 + u)^(n + 1) - 1) |scale| sum |a_i b_i| <= 1.01 (n + 2) u |scale| sum |a_i b_i|.
  merge     acc is a chain of `rank` fmas (error <= 1.01 rank u sum_k |B A|), then ONE fma rounds scale * acc + base:
            |err| <= 1.01 (rank + 1) u |scale| sum_k |B A| + u |result|.
No element is excused.
"""
import ctypes

import numpy as np
import pytest
import torch

from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.adapters import AdapterAdam, LowRankAdapters
from pytorchwavenetvocoder_amd.engine import _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import parity_common as PC
from tests.golden_util import GoldenCase

U24 = 2.0 ** -24
NAN_BITS = 0x7fc12345
# rows, cols, rank: straddling the 64 x 64 tile in both directions; the last two span several blocks in one direction only
SHAPES = [(2, 2, 1), (3, 5, 2), (8, 24, 3), (8, 24, 7), (12, 8, 7), (33, 65, 4), (64, 128, 8), (65, 127, 16), (130, 257, 5),
          (256, 64, 32), (128, 96, 64), (16, 2050, 2), (2050, 16, 2)]
SCALES = [1.0, 0.5, 2.0, -0.75, 1.0 / 3.0, 1.7]
GOLDEN = ["tiny_k2_up", "tiny_k3_noup"]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- op level ----------------------------------------------------------------------------------------------------------------
class Problem(object):
    """All SHAPES in one table.  Ranges are separated and surrounded by guard bands of at least 3 elements, and the gaps are
    chosen so that w_off, a_off and b_off each take every value modulo 4."""

    def __init__(self, scales=None):
        self.entries = []
        w = a = 3
        for i, (rows, cols, rank) in enumerate(SHAPES):
            scale = (SCALES[i % len(SCALES)] if scales is None else scales[i])
            while w % 4 != i % 4:
                w += 1
            w_off, w = w, w + rows * cols + 3
            first, second = ("A", "B") if i % 2 == 0 else ("B", "A")   # the two factors in either order
            offs = {}
            for which, want in ((first, (i + 1) % 4), (second, (i + 3) % 4)):
                while a % 4 != want:
                    a += 1
                offs[which] = a
                a += (rank * cols if which == "A" else rows * rank) + 3
            self.entries.append(dict(w_off=w_off, rows=rows, cols=cols, rank=rank, a_off=offs["A"], b_off=offs["B"], scale=scale))
        self.n_model, self.n_adapter = w + 5, a + 5
        for key in ("w_off", "a_off", "b_off"):
            assert {e[key] % 4 for e in self.entries} == {0, 1, 2, 3}, key

    def model_mask(self):
        m = np.zeros(self.n_model, bool)
        for e in self.entries:
            assert not m[e["w_off"]:e["w_off"] + e["rows"] * e["cols"]].any()
            m[e["w_off"]:e["w_off"] + e["rows"] * e["cols"]] = True
        return m

    def adapter_mask(self):
        m = np.zeros(self.n_adapter, bool)
        for e in self.entries:
            for off, n in ((e["a_off"], e["rank"] * e["cols"]), (e["b_off"], e["rows"] * e["rank"])):
                assert not m[off:off + n].any()
                m[off:off + n] = True
        return m

    def W(self, buf, e):
        return buf[e["w_off"]:e["w_off"] + e["rows"] * e["cols"]].reshape(e["rows"], e["cols"])

    def A(self, buf, e):
        return buf[e["a_off"]:e["a_off"] + e["rank"] * e["cols"]].reshape(e["rank"], e["cols"])

    def B(self, buf, e):
        return buf[e["b_off"]:e["b_off"] + e["rows"] * e["rank"]].reshape(e["rows"], e["rank"])


def _values(rs, n):
    """Normal values with magnitudes clamped into [1e-6, 1e6], and a sprinkling of +-1e6, +-1e-6 and exact zeros."""
    v = rs.standard_normal(n)
    v = np.sign(v) * np.clip(np.abs(v), 1e-6, 1e6)
    v[v == 0.0] = 1e-6
    pick = rs.uniform(size=n)
    sign = np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)
    v = np.where(pick < 0.02, sign * 1e6, v)
    v = np.where((pick >= 0.02) & (pick < 0.04), sign * 1e-6, v)
    v = np.where((pick >= 0.04) & (pick < 0.07), 0.0, v)
    return v.astype(np.float32)


def make_data(prob, seed=5):
    """(base, grads, adapter) as fp32 numpy buffers; outside the ranges they hold ordinary values too (nobody may read them, and
    nothing would show if somebody did -- the guard bands of the OUTPUT buffers do that job)."""
    rs = np.random.RandomState(seed)
    base, grads, adapter = _values(rs, prob.n_model), _values(rs, prob.n_model), _values(rs, prob.n_adapter)
    for e in prob.entries:
        g, a, b = prob.W(grads, e), prob.A(adapter, e), prob.B(adapter, e)
        if e["rows"] >= 2:      # rows that cancel in dA: g[1] = -g[0] under equal factors B[1] = B[0]
            g[1] = -g[0]
            b[1] = b[0]
        if e["cols"] >= 4:      # and in dB / in the merge: columns 2, 3
            g[:, 3] = g[:, 2]
            a[:, 3] = -a[:, 2]
    return base, grads, adapter


def build_table(lib, prob, dev, entries=None, n_model=None, n_adapter=None):
    """(host table, device table, scratch floats); asserts the two-call protocol of wn_lora_table."""
    entries = prob.entries if entries is None else entries
    arr = (_lib.WnLoraEntry * max(len(entries), 1))()
    for a, e in zip(arr, entries):
        for k, v in e.items():
            setattr(a, k, v)
    n_model = prob.n_model if n_model is None else n_model
    n_adapter = prob.n_adapter if n_adapter is None else n_adapter
    words = lib.wn_lora_table(ctypes.cast(arr, ctypes.c_void_p), len(entries), n_model, n_adapter, None, 0)
    if words < 0:
        return None
    host = torch.zeros(int(words), dtype=torch.int64)
    assert lib.wn_lora_table(ctypes.cast(arr, ctypes.c_void_p), len(entries), n_model, n_adapter, ctypes.c_void_p(host.data_ptr()),
                             int(words)) == words, lib.wn_last_error()
    return host, host.to(dev), int(lib.wn_lora_scratch_floats(ctypes.c_void_p(host.data_ptr())))


def nan_filled(n, dev):
    return torch.full((n,), NAN_BITS, dtype=torch.int32).view(torch.float32).to(dev)


def run_merge(lib, dev, prob, tab, base, adapter, params):
    lib.check(lib.wn_lora_merge(_ptr(base), _ptr(params), prob.n_model, _ptr(adapter), prob.n_adapter,
                                ctypes.c_void_p(tab[0].data_ptr()), _ptr(tab[1]), _stream_handle(torch.device(dev))), "wn_lora_merge")


def run_project(lib, dev, prob, tab, grads, adapter, out, scratch=None):
    scratch = nan_filled(tab[2] + 7, dev) if scratch is None else scratch
    lib.check(lib.wn_lora_project(_ptr(grads), prob.n_model, _ptr(adapter), _ptr(out), prob.n_adapter,
                                  ctypes.c_void_p(tab[0].data_ptr()), _ptr(tab[1]), _ptr(scratch), scratch.numel(),
                                  _stream_handle(torch.device(dev))), "wn_lora_project")


class OpRun(object):
    """One merge and one project of the whole table, computed once and shared by the op-level checks (never modified)."""
    _cache = {}

    @classmethod
    def get(cls, lib, dev):
        key = (lib.path, dev)
        if key not in cls._cache:
            cls._cache[key] = cls(lib, dev)
        return cls._cache[key]

    def __init__(self, lib, dev):
        self.prob = prob = Problem()
        self.tab = build_table(lib, prob, dev)
        self.np_base, self.np_grads, self.np_adapter = make_data(prob)
        self.base, self.grads, self.adapter = (torch.from_numpy(x.copy()).to(dev) for x in (self.np_base, self.np_grads, self.np_adapter))
        self.params, self.out = nan_filled(prob.n_model, dev), nan_filled(prob.n_adapter, dev)
        run_merge(lib, dev, prob, self.tab, self.base, self.adapter, self.params)
        run_project(lib, dev, prob, self.tab, self.grads, self.adapter, self.out)


def check_inputs_and_guard_bands(lib, dev):
    r = OpRun.get(lib, dev)
    for name, t, ref in (("base", r.base, r.np_base), ("grads", r.grads, r.np_grads), ("adapter", r.adapter, r.np_adapter)):
        assert same_bits(t, torch.from_numpy(ref)), "%s was written" % name
    for name, t, mask in (("params", r.params, r.prob.model_mask()), ("adapter_grads", r.out, r.prob.adapter_mask())):
        got = bits(t).numpy()
        assert (got[~mask] == NAN_BITS).all(), "%s: a guard band lost its bits" % name
        assert not np.isnan(t.cpu().numpy()[mask]).any(), "%s: an element of a range was not written" % name
        assert (~mask).sum() >= 3 * len(SHAPES)


def check_merge_bound(lib, dev, i):
    r = OpRun.get(lib, dev)
    e = r.prob.entries[i]
    s = np.float64(np.float32(e["scale"]))
    A, B, base = f64(r.prob.A(r.adapter, e)), f64(r.prob.B(r.adapter, e)), f64(r.prob.W(r.base, e))
    want = base + s * (B @ A)
    tol = 1.01 * (e["rank"] + 1) * U24 * abs(s) * (np.abs(B) @ np.abs(A)) + U24 * np.abs(want)
    err = np.abs(f64(r.prob.W(r.params, e)) - want)
    print("merge %s: max err / tol = %.3f" % (SHAPES[i], float((err / np.maximum(tol, 1e-300)).max())))
    assert (err <= tol).all(), SHAPES[i]


def check_project_bound(lib, dev, i):
    r = OpRun.get(lib, dev)
    e = r.prob.entries[i]
    s = np.float64(np.float32(e["scale"]))
    A, B, g = f64(r.prob.A(r.adapter, e)), f64(r.prob.B(r.adapter, e)), f64(r.prob.W(r.grads, e))
    for name, got, want, mag, n in (("dA", r.prob.A(r.out, e), s * (B.T @ g), np.abs(B).T @ np.abs(g), e["rows"]),
                                    ("dB", r.prob.B(r.out, e), s * (g @ A.T), np.abs(g) @ np.abs(A).T, e["cols"])):
        tol = 1.01 * (n + 2) * U24 * abs(s) * mag
        err = np.abs(f64(got) - want)
        print("project %s %s: max err / tol = %.3f" % (name, SHAPES[i], float((err / np.maximum(tol, 1e-300)).max())))
        assert (err <= tol).all(), (name, SHAPES[i])


def check_exact_invariants(lib, dev):
    r = OpRun.get(lib, dev)
    prob, tab, mask = r.prob, r.tab, torch.from_numpy(r.prob.model_mask())
    # B = 0: the merged weights are the base on the ranges
    zeroed = r.adapter.clone()
    for e in prob.entries:
        prob.B(zeroed, e).zero_()
    params = nan_filled(prob.n_model, dev)
    run_merge(lib, dev, prob, tab, r.base, zeroed, params)
    assert torch.equal(params.cpu()[mask], r.base.cpu()[mask])
    # merging twice gives the bits of merging once; two runs give identical bits
    params = r.params.clone()
    run_merge(lib, dev, prob, tab, r.base, r.adapter, params)
    assert same_bits(params, r.params)
    again = nan_filled(prob.n_model, dev)
    run_merge(lib, dev, prob, tab, r.base, r.adapter, again)
    assert same_bits(again, r.params)
    out = nan_filled(prob.n_adapter, dev)
    run_project(lib, dev, prob, tab, r.grads, r.adapter, out)
    assert same_bits(out, r.out)
    # (2 scale, A / 2): powers of two commute with every rounding, so the merge and dB keep their bits and dA doubles exactly
    twice = Problem(scales=[2.0 * e["scale"] for e in prob.entries])
    tab2 = build_table(lib, twice, dev)
    halved = r.adapter.clone()
    for e in prob.entries:
        prob.A(halved, e).mul_(0.5)
    params = nan_filled(prob.n_model, dev)
    run_merge(lib, dev, twice, tab2, r.base, halved, params)
    assert same_bits(params, r.params)
    out = nan_filled(prob.n_adapter, dev)
    run_project(lib, dev, twice, tab2, r.grads, halved, out)
    for e in prob.entries:
        assert same_bits(prob.B(out, e), prob.B(r.out, e))
        assert same_bits(prob.A(out, e), 2.0 * prob.A(r.out, e))
    # grads = 0: exact zeros
    out = nan_filled(prob.n_adapter, dev)
    run_project(lib, dev, prob, tab, torch.zeros_like(r.grads), r.adapter, out)
    assert bool((out.cpu()[torch.from_numpy(prob.adapter_mask())] == 0.0).all())


def check_argument_errors(lib, dev):
    prob = Problem()
    good = dict(w_off=8, rows=6, cols=10, rank=3, a_off=4, b_off=40, scale=1.0)

    def table_fails(text, n_model=100, n_adapter=100, **change):
        entries = change.pop("entries") if "entries" in change else [dict(good, **change)]
        assert build_table(lib, prob, dev, entries, n_model, n_adapter) is None, (text, change)
        assert text in lib.wn_last_error().decode(), (text, lib.wn_last_error())
    assert build_table(lib, prob, dev, [good], 100, 100) is not None
    table_fails("rank", rank=0)
    table_fails("rank", rank=65, rows=70, cols=70, n_model=10000, n_adapter=20000)
    table_fails("min(rows, cols)", rank=7)
    table_fails("rows", rows=0)
    table_fails("cols", cols=0)
    for bad in (float("inf"), float("nan"), 1e300):
        table_fails("finite", scale=bad)
    table_fails("model buffer", n_model=67)              # W ends at 68
    table_fails("model buffer", w_off=-1)
    table_fails("adapter buffer", n_adapter=57)          # B ends at 58
    table_fails("adapter buffer", a_off=-4)
    table_fails("adapter buffer", b_off=90)
    table_fails("overlap in the adapter buffer", b_off=33)    # A = [4, 34)
    table_fails("overlap in the model buffer", entries=[good, dict(good, w_off=67, a_off=60, b_off=80, rows=2, cols=4, rank=1)])
    table_fails("overlap in the adapter buffer", entries=[good, dict(good, w_off=70, a_off=57, b_off=80, rows=2, cols=4, rank=1)])
    table_fails("empty", entries=[])
    arr = (_lib.WnLoraEntry * 1)()
    assert lib.wn_lora_table(None, 1, 100, 100, None, 0) == -1 and "NULL" in lib.wn_last_error().decode()
    for k, v in good.items():
        setattr(arr[0], k, v)
    small = torch.zeros(4, dtype=torch.int64)
    assert lib.wn_lora_table(ctypes.cast(arr, ctypes.c_void_p), 1, 100, 100, ctypes.c_void_p(small.data_ptr()), 4) == -1
    assert "words" in lib.wn_last_error().decode()
    assert lib.wn_lora_scratch_floats(ctypes.c_void_p(small.data_ptr())) == -1 and lib.wn_lora_scratch_floats(None) == -1
    # the two launches
    host, devt, nscr = build_table(lib, prob, dev, [good], 100, 100)
    st = _stream_handle(torch.device(dev))
    base, params, grads = (torch.zeros(100, dtype=torch.float32, device=dev) for _ in range(3))
    adapter, out = (torch.zeros(100, dtype=torch.float32, device=dev) for _ in range(2))
    scratch = torch.zeros(nscr, dtype=torch.float32, device=dev)
    H, P = ctypes.c_void_p(host.data_ptr()), (lambda t: None if t is None else t.data_ptr())

    def merge(b=base, p=params, nm=100, a=adapter, na=100, h=H, d=devt):
        return lib.wn_lora_merge(P(b) if torch.is_tensor(b) else b, P(p) if torch.is_tensor(p) else p, nm, P(a), na, h, P(d), st)

    def project(g=grads, nm=100, a=adapter, o=out, na=100, h=H, d=devt, s=scratch, ns=None):
        o_ = P(o) if torch.is_tensor(o) or o is None else o
        return lib.wn_lora_project(P(g), nm, P(a), o_, na, h, P(d), P(s) if torch.is_tensor(s) or s is None else s,
                                   (0 if s is None else nscr) if ns is None else ns, st)

    def fails(rc, text):
        assert rc != 0 and text in lib.wn_last_error().decode(), (rc, text, lib.wn_last_error())
    assert merge() == 0 and project() == 0, lib.wn_last_error()
    for kw in (dict(b=None), dict(p=None), dict(a=None), dict(d=None)):
        fails(merge(**kw), "wn_lora_merge")
    for kw in (dict(g=None), dict(a=None), dict(o=None), dict(d=None), dict(s=None)):
        fails(project(**kw), "wn_lora_project")
    fails(merge(h=None), "table is NULL")
    fails(project(h=None), "table is NULL")
    fails(merge(h=ctypes.c_void_p(small.data_ptr())), "not what wn_lora_table wrote")
    fails(merge(b=base.data_ptr() + 2), "alignment")
    fails(merge(p=params.data_ptr() + 1), "alignment")
    fails(project(o=out.data_ptr() + 2), "alignment")
    fails(project(s=scratch.data_ptr() + 2), "alignment")
    fails(merge(nm=67), "model buffer length")
    fails(merge(na=57), "adapter buffer length")
    fails(project(nm=67), "model buffer length")
    fails(project(na=57), "adapter buffer length")
    fails(project(ns=nscr - 1), "scratch")
    fails(merge(p=base), "overlaps")
    fails(project(o=adapter), "overlaps")
    for t in (params, out):
        assert not bool(t.cpu().any())          # no refused call wrote anything


# ---- module level ----------------------------------------------------------------------------------------------------------------
def _model(name, lib, dev):
    g = GoldenCase(name)
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(dev)
    return g, model, g.x.to(dev), g.h.to(dev), g.t.to(dev)


def _randomize_B(ad, seed=9):
    gen = torch.Generator().manual_seed(seed)
    for v in ad.B.values():
        v.copy_((0.05 * torch.randn(v.shape, generator=gen)).to(v.device))


def _adapted_mask(ad):
    m = torch.zeros(ad.model.engine.n_params, dtype=torch.bool)
    for key, idx, w_off, rows, cols, a_off, b_off, shape in ad.entries:
        m[w_off:w_off + rows * cols] = True
    return m


def project_bound_check(ad, grads, got, what=""):
    """``got`` (a flat adapter-gradient buffer) against float64 matmuls of ``grads`` (a flat model-gradient buffer)."""
    s = np.float64(np.float32(ad.scale))
    flat, g_all, got = f64(ad.flat), f64(grads), f64(got)
    for key, idx, w_off, rows, cols, a_off, b_off, shape in ad.entries:
        r = ad.rank
        A, B = flat[a_off:a_off + r * cols].reshape(r, cols), flat[b_off:b_off + rows * r].reshape(rows, r)
        g = g_all[w_off:w_off + rows * cols].reshape(rows, cols)
        for name, have, want, mag, n in (("dA", got[a_off:a_off + r * cols].reshape(r, cols), s * (B.T @ g), np.abs(B).T @ np.abs(g), rows),
                                        ("dB", got[b_off:b_off + rows * r].reshape(rows, r), s * (g @ A.T), np.abs(g) @ np.abs(A).T, cols)):
            assert (np.abs(have - want) <= 1.01 * (n + 2) * U24 * abs(s) * mag).all(), (what, key, name)


def check_fresh_adapters(name, lib, dev):
    g, model, x, h, t = _model(name, lib, dev)
    eng = model.engine
    p0 = eng.flat_params.cpu().clone()
    ad = LowRankAdapters(model, rank=2)
    keys = [k for k, _ in model.named_parameters()]
    L = len(g.cfg.dilations)
    want = [k for k in keys if k.split(".")[0] in ("dil_sigmoid", "dil_tanh", "skip_1x1", "res_1x1") and k.endswith("weight")
            and k != "res_1x1.%d.weight" % (L - 1)]
    assert ad.keys == want and len(want) == 4 * L - 1
    assert [k for k, p in model.named_parameters() if p.requires_grad] == want
    assert same_bits(ad.base, p0) and ad.flat.numel() == sum(a.numel() + b.numel() for a, b in zip(ad.A.values(), ad.B.values()))
    assert all(not bool(b.any()) for b in ad.B.values()) and all(bool(a.any()) for a in ad.A.values())
    twin = LowRankAdapters(_model(name, lib, dev)[1], rank=2)
    assert same_bits(twin.flat, ad.flat)                       # ranks start identical without communication
    assert not same_bits(LowRankAdapters(_model(name, lib, dev)[1], rank=2, seed=1).flat, ad.flat)
    eng.flat_params.fill_(float("nan"))
    eng.flat_params[~_adapted_mask(ad).to(dev)] = p0.to(dev)[~_adapted_mask(ad).to(dev)]
    v = eng.params_version()
    ad.merge()
    assert eng.params_version() != v
    assert torch.equal(eng.flat_params.cpu(), p0)              # B = 0: the pretrained weights
    assert same_bits(eng.flat_params.cpu()[~_adapted_mask(ad)], p0[~_adapted_mask(ad)])


def check_targets(lib, dev):
    def fresh():
        return _model("tiny_k2_up", lib, dev)[1]
    for targets, word in ((r"skip_1x1\.0\.", "skip_1x1.0.bias"), (r"nothing_like_this", "matches no parameter"),
                          (r"upsampling\.conv\.weight", "upsampling.conv.weight")):
        with pytest.raises(ValueError, match=word.replace(".", r"\.")):
            LowRankAdapters(fresh(), rank=2, targets=targets)
    with pytest.raises(ValueError):
        LowRankAdapters(fresh(), rank=0)
    with pytest.raises(ValueError):
        LowRankAdapters(fresh(), rank=65)
    ad = LowRankAdapters(fresh(), rank=3, alpha=6.0, targets=r"^(aux_1x1_sigmoid\.1|conv_post_1)\.weight$")
    assert ad.keys == ["aux_1x1_sigmoid.1.weight", "conv_post_1.weight"] and ad.scale == 2.0
    L = ad.model.engine.n_layers
    assert "res_1x1.%d.weight" % (L - 1) not in LowRankAdapters(fresh(), rank=2, targets=r"res_1x1\.\d+\.weight").keys


def check_project(name, lib, dev):
    g, model, x, h, t = _model(name, lib, dev)
    eng = model.engine
    ad = LowRankAdapters(model, rank=3, alpha=1.5)
    _randomize_B(ad)
    ad.merge()
    with pytest.raises(RuntimeError, match="no gradient"):
        ad.project()
    bias_key = "skip_1x1.0.bias"
    bias = dict(model.named_parameters())[bias_key]
    bias.requires_grad_(True)
    model.loss_and_backward(x, h, t)
    grads = eng.grads().cpu().clone()
    flat0 = ad.flat.detach().cpu().clone()
    ad.project()
    assert same_bits(eng.grads(), grads) and same_bits(ad.flat, flat0)
    project_bound_check(ad, grads, ad.flat.grad, name)
    assert float(ad.flat.grad.abs().max()) > 0.0
    adapted = set(ad.keys)
    for k, p in model.named_parameters():
        assert (p.grad is None) == (k != bias_key), k
    with pytest.raises(RuntimeError, match="no gradient"):
        ad.project()                                            # once per gradient
    # FusedAdam, by its rule, leaves every tensor without a gradient alone: only the bias moves
    w0 = eng.flat_params.cpu().clone()
    opt = FusedAdam(model, lr=1e-2)
    opt.step()
    w1 = eng.flat_params.cpu()
    off, n, _, _ = model._param_slices[[k for k, _ in model.named_parameters()].index(bias_key)]
    moved = torch.zeros(eng.n_params, dtype=torch.bool)
    moved[off:off + n] = True
    assert same_bits(w1[~moved], w0[~moved]) and not same_bits(w1[moved], w0[moved]) and adapted
    # a frozen adapted tensor
    model.loss_and_backward(x, h, t)
    dict(model.named_parameters())[ad.keys[0]].requires_grad_(False)
    with pytest.raises(RuntimeError, match="frozen"):
        ad.project()


def check_training(name, lib, dev):
    g, model, x, h, t = _model(name, lib, dev)
    eng = model.engine
    p0 = eng.flat_params.cpu().clone()
    ad = LowRankAdapters(model, rank=2)
    opt = AdapterAdam(ad, lr=5e-3)
    assert (opt.guarded, opt.grad_norm, opt.ema_decay, opt.steps_skipped()) == (False, None, None, 0)
    losses = []
    for _ in range(20):
        losses.append(model.loss_and_backward(x, h, t))
        ad.project()
        opt.step()
    losses = [float(v) for v in losses]
    print("%s: loss %.5f -> %.5f" % (name, losses[0], losses[-1]))
    assert losses[-1] < losses[0] and opt.steps_applied() == 20
    mask = _adapted_mask(ad)
    w = eng.flat_params.cpu()
    assert same_bits(ad.base, p0) and same_bits(w[~mask], p0[~mask]) and not same_bits(w[mask], p0[mask])
    ad.restore()
    assert same_bits(eng.flat_params, p0)
    ad.merge()
    assert same_bits(eng.flat_params, w)


def check_step_bits(lib, dev):
    g, model, x, h, t = _model("tiny_k2_up", lib, dev)
    eng = model.engine
    kw = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-2)
    ad = LowRankAdapters(model, rank=2)
    _randomize_B(ad)
    ad.merge()
    opt = AdapterAdam(ad, **kw)
    st = _stream_handle(torch.device(dev))
    p, m, v = ad.flat.detach().clone(), torch.zeros_like(ad.flat.data), torch.zeros_like(ad.flat.data)
    for step in (1, 2):
        model.loss_and_backward(x, h, t)
        ad.project()
        lib.check(lib.wn_adam_step(_ptr(p), _ptr(ad.flat.grad), _ptr(m), _ptr(v), p.numel(), step, kw["lr"], kw["betas"][0],
                                   kw["betas"][1], kw["eps"], kw["weight_decay"], 0, 0, st), "wn_adam_step")
        opt.step()
        assert same_bits(ad.flat, p) and same_bits(opt._exp_avg, m) and same_bits(opt._exp_avg_sq, v), step
        params = nan_filled(eng.n_params, dev)
        rc = lib.wn_lora_merge(_ptr(ad.base), _ptr(params), eng.n_params, _ptr(p), p.numel(), ctypes.c_void_p(ad._table.data_ptr()),
                               _ptr(ad._dev_table), st)
        lib.check(rc, "wn_lora_merge")
        mask = _adapted_mask(ad)
        assert same_bits(params.cpu()[mask], eng.flat_params.cpu()[mask])   # the step ended with the merge
    # guarded: an inf in the adapter's gradient changes nothing and is counted
    gopt = AdapterAdam(ad, skip_nonfinite=True, max_grad_norm=0.5, **kw)
    model.loss_and_backward(x, h, t)
    ad.project()
    gopt.step()
    assert (gopt.steps_applied(), gopt.steps_skipped()) == (1, 0) and float(gopt.grad_norm) > 0.0
    before = [z.cpu().clone() for z in (ad.flat.detach(), gopt._exp_avg, gopt._exp_avg_sq, eng.flat_params)]
    model.loss_and_backward(x, h, t)
    ad.project()
    ad.flat.grad[ad.flat.numel() // 2] = float("inf")
    gopt.step()
    assert (gopt.steps_applied(), gopt.steps_skipped()) == (1, 1)
    for a, b in zip(before, (ad.flat.detach(), gopt._exp_avg, gopt._exp_avg_sq, eng.flat_params)):
        assert same_bits(a, b)
    with pytest.raises(RuntimeError):
        AdapterAdam(LowRankAdapters(_model("tiny_k2_up", lib, dev)[1], rank=2)).step()   # no project() yet
    for bad in (dict(ema_decay=0.99), dict(groups=[("x", {})]), dict(layer_adaptation=True)):
        with pytest.raises(ValueError, match="adapters"):
            AdapterAdam(ad, **bad)


def check_checkpoint(lib, dev, tmp_path):
    g, model, x, h, t = _model("tiny_k2_up", lib, dev)
    kw = dict(lr=2e-3, weight_decay=1e-3)
    ad = LowRankAdapters(model, rank=2, alpha=3.0)
    opt = AdapterAdam(ad, **kw)
    for _ in range(2):
        model.loss_and_backward(x, h, t)
        ad.project()
        opt.step()
    sd, osd = ad.state_dict(), opt.state_dict()
    assert set(sd.keys()) == {"rank", "alpha", "targets", "config", "A", "B"}
    assert [k for k, _ in sd["targets"]] == ad.keys == list(sd["A"].keys()) == list(sd["B"].keys())
    assert set(osd.keys()) == {"state", "param_groups"} and set(osd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}
    path = str(tmp_path / "adapter.pkl")
    torch.save({"adapter": sd, "optimizer": osd}, path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    g2, other, _, _, _ = _model("tiny_k2_up", lib, dev)         # a new model from the same base
    ad2 = LowRankAdapters(other, rank=2, seed=77)
    ad2.load_state_dict(ck["adapter"])
    ad2.merge()
    assert ad2.alpha == 3.0 and same_bits(ad2.flat, ad.flat) and same_bits(other.engine.flat_params, model.engine.flat_params)
    opt2 = AdapterAdam(ad2, **kw)
    opt2.load_state_dict(ck["optimizer"])
    for mdl, a, o in ((model, ad, opt), (other, ad2, opt2)):
        mdl.loss_and_backward(x, h, t)
        a.project()
        o.step()
    assert same_bits(ad2.flat, ad.flat) and same_bits(other.engine.flat_params, model.engine.flat_params)
    assert same_bits(opt2._exp_avg, opt._exp_avg) and same_bits(opt2._exp_avg_sq, opt._exp_avg_sq) and opt2.steps_applied() == 3
    ref = torch.nn.Parameter(ad.flat.detach().cpu().clone())
    topt = torch.optim.Adam([ref], **kw)
    topt.load_state_dict(ck["optimizer"])                      # torch.optim.Adam's format for the single parameter
    assert torch.equal(topt.state[ref]["exp_avg"], ck["optimizer"]["state"][0]["exp_avg"])
    # mismatches
    for change in (dict(rank=3), dict(config=dict(sd["config"], n_resch=sd["config"]["n_resch"] + 1)),
                   dict(targets=sd["targets"][1:]), dict(targets=[(k, tuple(s) + (1,)) for k, s in sd["targets"]])):
        with pytest.raises(ValueError):
            ad2.load_state_dict(dict(sd, **change))
    with pytest.raises(ValueError):
        LowRankAdapters(_model("tiny_k2_up", lib, dev)[1], rank=3).load_state_dict(sd)
    with pytest.raises(ValueError):
        LowRankAdapters(_model("tiny_k3_noup", lib, dev)[1], rank=2).load_state_dict(sd)
    badA = dict(sd, A={k: v[:, :-1] for k, v in sd["A"].items()})
    with pytest.raises(ValueError):
        ad2.load_state_dict(badA)


def check_fold(lib, dev):
    g, model, x, h, t = _model("tiny_k3_noup", lib, dev)
    ad = LowRankAdapters(model, rank=2)
    _randomize_B(ad)
    ad.fold()
    merged = model.state_dict()
    assert all(p.requires_grad for p in model.parameters())
    for call in (ad.merge, ad.project, ad.restore):
        with pytest.raises(RuntimeError, match="folded"):
            call()
    plain = WaveNet(*g.cfg.as_tuple(), _library=lib)
    plain.load_state_dict(merged)
    plain.to(dev)
    opts = [FusedAdam(m, lr=1e-3) for m in (model, plain)]
    for m, o in zip((model, plain), opts):
        loss = m.loss_and_backward(x, h, t)
        o.step()
    assert same_bits(model.engine.flat_params, plain.engine.flat_params)   # it trains as a plain model does, every tensor
    assert same_bits(model.loss_and_backward(x, h, t), plain.loss_and_backward(x, h, t))


def check_launches(lib, dev):
    g, model, x, h, t = _model("tiny_k2_up", lib, dev)
    ad = LowRankAdapters(model, rank=2)
    for kw, want in ((dict(), {"adam": 1, "lora_merge": 1}),
                     (dict(max_grad_norm=0.05, skip_nonfinite=True),
                      {"grad_sumsq": 1, "grad_norm_finalize": 1, "adam_guarded": 1, "lora_merge": 1})):
        opt = AdapterAdam(ad, lr=1e-3, **kw)
        for _ in range(2):
            model.loss_and_backward(x, h, t)
            assert PC.launch_log(lib, ad.project) == {"lora_partials": 1, "lora_reduce": 1}
            log = PC.launch_log(lib, opt.step)
            assert log == want, (kw, log)
    assert PC.launch_log(lib, ad.merge) == {"lora_merge": 1}


def check_micro_steps(lib, dev):
    g, model, x, h, t = _model("tiny_k2_up", lib, dev)
    eng = model.engine
    ad = LowRankAdapters(model, rank=2, alpha=3.0)
    _randomize_B(ad)
    ad.merge()
    halves = [(x[:1], h[:1], t[:1]), (x[1:], h[1:], t[1:])] if x.shape[0] > 1 else [(x, h, t), (x, h, t)]
    parts, gs = [], []
    for xb, hb, tb in halves:                                   # the two micro-batches on their own
        model.loss_and_backward(xb, hb, tb, grad_scale=0.5)
        gs.append(eng.grads().cpu().clone())
        ad.project()
        parts.append(ad.flat.grad.cpu().clone())
    model.loss_and_backward(*halves[0], grad_scale=0.5, micro_step=(0, 2))
    with pytest.raises(RuntimeError, match="accumulation"):
        ad.project()
    model.loss_and_backward(*halves[1], grad_scale=0.5, micro_step=(1, 2))
    summed = eng.grads().cpu().clone()
    ad.project()
    got = ad.flat.grad.cpu().clone()
    project_bound_check(ad, summed, got, "sum")
    # against the sum of the two projections: each of the three projections is inside its bound, the gradient sum rounded once
    # per element (u |g0 + g1| before the contraction) and so does the sum of the two projections (u |sum|)
    s = abs(np.float64(np.float32(ad.scale)))
    flat = f64(ad.flat)
    have, want = f64(got), f64(parts[0]) + f64(parts[1])
    for key, idx, w_off, rows, cols, a_off, b_off, shape in ad.entries:
        r = ad.rank
        A, B = np.abs(flat[a_off:a_off + r * cols].reshape(r, cols)), np.abs(flat[b_off:b_off + rows * r].reshape(rows, r))
        mags = [np.abs(f64(z)[w_off:w_off + rows * cols].reshape(rows, cols)) for z in (gs[0], gs[1], summed)]
        for off, n, n_red, mag in ((a_off, r * cols, rows, [B.T @ m for m in mags]), (b_off, rows * r, cols, [m @ A.T for m in mags])):
            tol = sum(1.01 * (n_red + 2) * U24 * s * m for m in mag) + U24 * s * (mag[0] + mag[1]) + U24 * np.abs(want[off:off + n].reshape(mag[0].shape))
            assert (np.abs(have[off:off + n] - want[off:off + n]).reshape(mag[0].shape) <= tol).all(), key
