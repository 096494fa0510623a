# -*- coding: utf-8 -*-
"""Op-level matrix of wn_op_gemm (csrc/wn_gemm.hip): an fp64 restatement of include/wavenet_hip_gemm.h, a case builder
that puts every operand between NaN guard bands, and a predictor of the staging paths a launch takes.

Three independent parts:
  * ``reference``      the header's formula, element by element, as vectorised NumPy gathers in fp64.  It knows nothing
                       of tiles, staging paths or the kernel's pointer walk.
  * ``build_case``     allocations: every operand is a slice of a larger tensor.  Whatever the header does not name as
                       an element of the operand (guard bands, the gaps a leading dimension or a stride leaves) holds
                       NaN, so a read outside the operand shows as NaN in the result instead of going unnoticed.
                       C and a_rowsum live in sentinel-filled tensors whose non-result elements must survive bit for bit.
  * ``predict_paths``  the kernel's block-uniform predicates restated per block and k-tile -> the set of labels a launch
                       exercises.  The matrix is complete when the union of the labels over CASES is ALL_LABELS.

Two data modes per case:
  exact    small integers: every product and partial sum is exact in fp32 in any order -> torch.equal, no tolerance
  rounded  standard-normal operands, elementwise |got - ref64| <= (Kz + 4) 2^-24 (sum_k |A||B| + |bias| + |D| + |C_old|):
           the forward error bound of a length-Kz fp32 dot product in any summation order ((Kz - 1) roundings of
           partial sums + 1 of each product, first order, with gamma_n <= n u) plus the epilogue's three additions.
"""
import types
import zlib

import numpy as np
import torch

from tests.gemm_util import run_gemm

GUARD = 1024                 # elements of guard band on each side of every operand
BIG = 0x7fffffff
SENTINEL = 0x7fc5a5a5        # bit pattern (a NaN with a payload) of every C / a_rowsum element that is no result
U = 2.0 ** -24               # fp32 unit roundoff
WN_BK = 32



def up4(x):
    return (int(x) + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------------------------
# the argument block of a case
# ------------------------------------------------------------------------------------------------------------------
DEFAULTS = dict(mode="fwd", M=64, N=64, K=64, lda=None, a_zstride=None, ldb=None, b_zstride=None, seg_len=None,
                seg_stride=0, shift0=0, shift_step=0, clen=None, b_relu=0, onehot=None, index_zstride=None,
                ldc=None, c_zstride=None, bias=0, D=0, d_in_place=0, ldd=None, E=0, lde=None, relu=0, accumulate=0,
                nbatch=1, ksplit=1, kchunk=None, rowsum=0, nlayer=1, a_lstride=None, b_lstride=None, dil_depth=0,
                layer0=0, a_off=0, b_off=0, fence_a=0)


def make_args(spec):
    """The integer fields of WnGemmArgs for a case; unspecified strides are the operand's extent rounded up to 4."""
    s = dict(DEFAULTS)
    unknown = set(spec) - set(s) - {"name"}
    assert not unknown, unknown
    s.update(spec)
    g = types.SimpleNamespace()
    kmaj = 1 if s["mode"] == "dw" else 0
    g.M, g.N, g.K = s["M"], s["N"], s["K"]
    g.a_kmajor = g.b_kmajor = kmaj
    g.b_seg_len = s["seg_len"] or BIG
    g.b_clen = s["clen"] if s["clen"] is not None else (g.K if kmaj else g.N)
    g.b_shift0, g.b_shift_step, g.b_relu = s["shift0"], s["shift_step"], s["b_relu"]
    g.onehot = s["onehot"]
    rows = g.N if kmaj else g.K                      # rows of the B operand
    nseg = max(1, -(-rows // g.b_seg_len))
    rows_per_seg = min(rows, g.b_seg_len)
    g.lda = s["lda"] if s["lda"] is not None else up4(g.K if kmaj else g.M)
    ext_a = ((g.M - 1) * g.lda + g.K) if kmaj else ((g.K - 1) * g.lda + g.M if g.K > 0 else 0)
    g.a_zstride = s["a_zstride"] if s["a_zstride"] is not None else up4(ext_a)
    g.nbatch, g.ksplit, g.nlayer = s["nbatch"], s["ksplit"], s["nlayer"]
    g.kchunk = s["kchunk"] or BIG
    g.a_lstride = s["a_lstride"] if s["a_lstride"] is not None else g.nbatch * g.a_zstride
    if g.onehot:
        g.b_seg_len = g.onehot
        g.b_index_mod = g.onehot
        g.ldb = g.b_seg_stride = g.b_zstride = g.b_lstride = 0
        g.b_index_zstride = s["index_zstride"] if s["index_zstride"] is not None else g.b_clen + 5
    else:
        g.b_index_mod, g.b_index_zstride = 1, 0
        g.ldb = s["ldb"] if s["ldb"] is not None else up4(g.b_clen)
        g.b_seg_stride = s["seg_stride"]
        ext_b = ((nseg - 1) * g.b_seg_stride + (rows_per_seg - 1) * g.ldb + g.b_clen) if rows > 0 else 0
        g.b_zstride = s["b_zstride"] if s["b_zstride"] is not None else up4(ext_b)
        g.b_lstride = s["b_lstride"] if s["b_lstride"] is not None else g.nbatch * g.b_zstride
    g.b_dil_depth, g.b_layer0 = s["dil_depth"], s["layer0"]
    g.ldc = s["ldc"] if s["ldc"] is not None else g.N
    g.c_zstride = s["c_zstride"] if s["c_zstride"] is not None else g.M * g.ldc
    g.has_bias, g.has_D, g.has_E, g.has_rowsum = bool(s["bias"]), bool(s["D"] or s["d_in_place"]), bool(s["E"]), bool(s["rowsum"])
    g.d_in_place = bool(s["d_in_place"])
    if g.d_in_place:
        assert g.ksplit == 1 and g.nlayer == 1 and not s["accumulate"]      # D follows b, C follows z: in place needs z == b
        g.ldd, g.d_zstride = g.ldc, g.c_zstride
    else:
        g.ldd = s["ldd"] if s["ldd"] is not None else g.N + 1
        g.d_zstride = g.M * g.ldd
    g.lde = s["lde"] if s["lde"] is not None else g.N + 2
    g.e_zstride = g.M * g.lde + 7
    g.relu, g.accumulate = s["relu"], s["accumulate"]
    g.a_off, g.b_off = s["a_off"], s["b_off"]
    g.nz = g.nlayer * g.nbatch * g.ksplit
    return g


# ------------------------------------------------------------------------------------------------------------------
# the reference: include/wavenet_hip_gemm.h restated
# ------------------------------------------------------------------------------------------------------------------
def a_index(g, li, b):
    """[M, K] element offsets of A(m, k) of layer li, batch b relative to g.A (header: a_kmajor)."""
    m = np.arange(g.M, dtype=np.int64)[:, None]
    k = np.arange(g.K, dtype=np.int64)[None, :]
    e = (m * g.lda + k) if g.a_kmajor else (k * g.lda + m)
    return li * g.a_lstride + b * g.a_zstride + e


def b_index(g, li, b):
    """Element offsets (relative to g.B, or to g.b_index for the one-hot operand), validity and in-segment row of every
    B(k, n) of layer li, batch b, each as a [K, N] array (header: segments, shifts, b_clen, the layer's dilation)."""
    rows, cols = (g.N, g.K) if g.b_kmajor else (g.K, g.N)
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    seg, rr = r // g.b_seg_len, r % g.b_seg_len
    dil = 2 ** ((g.b_layer0 + li) % g.b_dil_depth) if g.b_dil_depth > 0 else 1
    cc = c - (g.b_shift0 + seg * g.b_shift_step) * dil
    valid = (cc >= 0) & (cc < g.b_clen)
    if g.onehot:
        idx = b * g.b_index_zstride + cc
    else:
        idx = li * g.b_lstride + b * g.b_zstride + seg * g.b_seg_stride + rr * g.ldb + cc
    rr = np.broadcast_to(rr, idx.shape)
    if g.b_kmajor:
        idx, valid, rr = idx.T, valid.T, rr.T
    return idx, valid, rr


def b_operand(g, li, b, Bflat, index_flat):
    idx, valid, rr = b_index(g, li, b)
    safe = np.where(valid, idx, 0)
    if g.onehot:
        if index_flat.size == 0:
            return np.zeros(idx.shape)
        q = index_flat[safe] % g.b_index_mod                # NumPy's % is the mathematical (non-negative) residue
        return np.where(valid & (q == rr), 1.0, 0.0)
    if Bflat.size == 0:
        return np.zeros(idx.shape)
    v = np.where(valid, Bflat[safe], 0.0)
    return np.maximum(v, 0.0) if g.b_relu else v


def reference(g, A, B, index, bias, D, E, C_old):
    """fp64 result of the call.  A, B, index: flat arrays addressed from the operand's base pointer; bias [M];
    D, E [nbatch, M, N] or None; C_old [nz, M, N] or None.
    Returns C [nz, M, N], the bound's magnitude sum [nz, M, N], the k length [nz], a_rowsum [nz, M] and its magnitude sum."""
    C = np.zeros((g.nz, g.M, g.N))
    mag = np.zeros((g.nz, g.M, g.N))
    rows, rmag, kz = np.zeros((g.nz, g.M)), np.zeros((g.nz, g.M)), np.zeros(g.nz, dtype=np.int64)
    for li in range(g.nlayer):
        for b in range(g.nbatch):
            Am = A[a_index(g, li, b)] if g.K > 0 else np.zeros((g.M, 0))
            Bm = b_operand(g, li, b, B, index)
            for ks in range(g.ksplit):
                z = (li * g.nbatch + b) * g.ksplit + ks
                k0, k1 = ks * g.kchunk, min(g.K, (ks + 1) * g.kchunk)
                k0 = min(k0, k1)
                kz[z] = k1 - k0
                v = Am[:, k0:k1] @ Bm[k0:k1]
                s = np.abs(Am[:, k0:k1]) @ np.abs(Bm[k0:k1])
                rows[z], rmag[z] = Am[:, k0:k1].sum(1), np.abs(Am[:, k0:k1]).sum(1)
                if bias is not None:
                    v = v + bias[:, None]
                    s = s + np.abs(bias)[:, None]
                if D is not None:
                    v = v + D[b]
                    s = s + np.abs(D[b])
                if g.relu:
                    v = np.maximum(v, 0.0)
                if E is not None:
                    v = np.where(E[b] > 0, v, 0.0)
                if C_old is not None:
                    v = v + C_old[z]
                    s = s + np.abs(C_old[z])
                C[z], mag[z] = v, s
    return C, mag, kz, rows, rmag


# ------------------------------------------------------------------------------------------------------------------
# allocations
# ------------------------------------------------------------------------------------------------------------------
def _values(rng, n, data):
    if data == "exact":
        return rng.integers(-3, 4, size=n).astype(np.float32)
    return rng.standard_normal(n).astype(np.float32)


def _guarded(payload, off, guard=GUARD):
    """payload between NaN guard bands, starting `off` (0..3) floats past a 16-byte boundary.  Returns (tensor, start)."""
    t = torch.full((guard + 4 + payload.size + guard,), float("nan"), dtype=torch.float32)
    start = guard + off
    t[start:start + payload.size] = torch.from_numpy(np.ascontiguousarray(payload, dtype=np.float32))
    return t, start


def _fenced(payload):
    """payload behind a NaN guard band and ending exactly at an inaccessible page: on the host a read past the operand's end
    stops the process, also where the value read could not reach the result (rows past M feed only rows that are not stored).
    Returns (tensor, start, the mapping that owns the memory)."""
    import ctypes
    import mmap
    page = mmap.PAGESIZE
    assert payload.size % 4 == 0
    body = (4 * (GUARD + payload.size) + page - 1) // page * page
    mm = mmap.mmap(-1, body + page)
    addr = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    rc = libc.mprotect(ctypes.c_void_p(addr + body), ctypes.c_size_t(page), 0)          # PROT_NONE
    assert rc == 0, ctypes.get_errno()
    t = torch.frombuffer(memoryview(mm)[:body], dtype=torch.float32)
    t.fill_(float("nan"))
    start = body // 4 - payload.size
    t[start:] = torch.from_numpy(np.ascontiguousarray(payload, dtype=np.float32))
    return t, start, mm


def _sentinel_tensor(n):
    t = torch.empty(n, dtype=torch.float32)
    t.view(torch.int32).fill_(SENTINEL)
    return t


def _strided(nb, M, N, ld, zstride):
    """element offsets of [nb, M, N] with the given leading dimension and slab stride"""
    return (np.arange(nb, dtype=np.int64)[:, None, None] * zstride + np.arange(M, dtype=np.int64)[None, :, None] * ld +
            np.arange(N, dtype=np.int64)[None, None, :])


class Case(object):
    pass


def build_case(spec, data):
    g = make_args(spec)
    rng = np.random.default_rng(zlib.crc32((spec["name"] + "/" + data).encode()))
    c = Case()
    c.g, c.name, c.data = g, spec["name"], data
    sel = zlib.crc32(spec["name"].encode())          # base-pointer offsets of the operands that take no staging path

    # A and B: values exactly at the offsets the header names, NaN everywhere else (gaps of lda / ldb / strides too)
    def fill(index_sets):
        used = np.unique(np.concatenate([i.ravel() for i in index_sets])) if index_sets else np.zeros(0, dtype=np.int64)
        assert used.size == 0 or used[0] >= 0
        flat = np.full(int(used[-1]) + 1 if used.size else 0, np.nan, dtype=np.float32)
        flat[used] = _values(rng, used.size, data)
        return flat

    lb = [(li, b) for li in range(g.nlayer) for b in range(g.nbatch)]
    c.A = fill([a_index(g, li, b) for li, b in lb]) if g.K > 0 else np.zeros(0, dtype=np.float32)
    c.index = np.zeros(0, dtype=np.int64)
    if g.onehot:
        c.B = np.zeros(0, dtype=np.float32)
        sets = []
        for li, b in lb:
            idx, valid, _ = b_index(g, li, b)
            sets.append(idx[valid])
        used = np.unique(np.concatenate(sets)) if sets else np.zeros(0, dtype=np.int64)
        n = int(used[-1]) + 1 if used.size else 0
        # gaps and guards: consecutive elements take consecutive residues, so an over-read of a run along k marks a
        # different row of the tile at every k
        c.index = _index_guard(np.arange(n, dtype=np.int64), g.b_index_mod)
        c.index[used] = rng.integers(-g.onehot, 3 * g.onehot, size=used.size)          # [-Q, 3Q)
    else:
        sets = []
        for li, b in lb:
            idx, valid, _ = b_index(g, li, b)
            sets.append(idx[valid])
        c.B = fill(sets)
    c.bias = _values(rng, g.M, data) if g.has_bias else None
    c.E = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32), size=(g.nbatch, g.M, g.N)) if g.has_E else None
    c.C_old = _values(rng, g.nz * g.M * g.N, data).reshape(g.nz, g.M, g.N) if g.accumulate else None
    c.D = _values(rng, g.nbatch * g.M * g.N, data).reshape(g.nbatch, g.M, g.N) if g.has_D else None

    f64 = lambda x: None if x is None else x.astype(np.float64)  # noqa: E731
    c.ref, c.mag, c.kz, c.ref_rows, c.rows_mag = reference(g, f64(c.A), f64(c.B), c.index, f64(c.bias), f64(c.D), f64(c.E),
                                                           f64(c.C_old))

    # ---- host tensors -------------------------------------------------------------------------------------------
    c.fence = bool(spec.get("fence_a"))          # host runs only (run_case); this tensor is guarded on both sides like every other
    c.tA, c.sA = _guarded(c.A, g.a_off)
    c.tB, c.sB = _guarded(c.B, g.b_off)
    assert c.tA.data_ptr() % 16 == 0 and c.tB.data_ptr() % 16 == 0
    c.tI = c.sI = None
    if g.onehot:
        ioff = sel % 2
        n = c.index.size
        full = _index_guard(np.arange(-(GUARD + ioff), n + GUARD, dtype=np.int64), g.b_index_mod)
        full[GUARD + ioff:GUARD + ioff + n] = c.index
        c.tI, c.sI = torch.from_numpy(full), GUARD + ioff
    c.tbias = c.sbias = c.tD = c.sD = c.tE = c.sE = None
    if g.has_bias:
        c.tbias, c.sbias = _guarded(c.bias, (sel >> 2) % 4)
    if g.has_E:
        pay = np.full((g.nbatch - 1) * g.e_zstride + (g.M - 1) * g.lde + g.N, np.nan, dtype=np.float32)
        pay[_strided(g.nbatch, g.M, g.N, g.lde, g.e_zstride)] = c.E
        c.tE, c.sE = _guarded(pay, (sel >> 4) % 4)
    if g.has_D and not g.d_in_place:
        pay = np.full((g.nbatch - 1) * g.d_zstride + (g.M - 1) * g.ldd + g.N, np.nan, dtype=np.float32)
        pay[_strided(g.nbatch, g.M, g.N, g.ldd, g.d_zstride)] = c.D
        # D follows the batch index b; room for an index by z to stay inside the allocation (it then reads NaN)
        c.tD, c.sD = _guarded(pay, (sel >> 6) % 4, guard=GUARD + (g.nz - g.nbatch) * g.d_zstride)
    # C: sentinel everywhere; result elements NaN (a skipped store shows), or the old C / the in-place D
    c.sC = GUARD + (sel >> 8) % 4
    c.c_idx = torch.from_numpy(_strided(g.nz, g.M, g.N, g.ldc, g.c_zstride) + c.sC)
    c.tC = _sentinel_tensor(c.sC + (g.nz - 1) * g.c_zstride + (g.M - 1) * g.ldc + g.N + GUARD)
    init = c.C_old if g.accumulate else (c.D if g.d_in_place else np.full((g.nz, g.M, g.N), np.nan, dtype=np.float32))
    c.tC[c.c_idx] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32))
    c.tR = None
    if g.has_rowsum:
        c.sR = GUARD + (sel >> 10) % 4
        c.tR = _sentinel_tensor(c.sR + g.nz * g.M + GUARD)
        c.tR[c.sR:c.sR + g.nz * g.M] = float("nan")
    return c


def _index_guard(pos, mod):
    return pos % mod + mod * ((pos // 3) % 5 - 2)          # residues cycle; multiples of mod added, negative ones too


def run_case(lib, device, spec, data):
    """Run one case of the matrix and assert on it.  Returns the worst error / bound ratio (0 in the exact mode)."""
    c = build_case(spec, data)
    g = c.g
    dev = {}

    def ptr(name, t, start):
        if t is None:
            return 0
        d = t.clone() if device == "cpu" else t.to(device)       # never the host original: it is compared with afterwards
        dev[name] = d
        return d.data_ptr() + start * t.element_size()

    kw = dict(M=g.M, N=g.N, K=g.K, lda=g.lda, a_zstride=g.a_zstride, a_kmajor=g.a_kmajor, ldb=g.ldb, b_zstride=g.b_zstride,
              b_kmajor=g.b_kmajor, b_seg_len=g.b_seg_len, b_seg_stride=g.b_seg_stride, b_shift0=g.b_shift0,
              b_shift_step=g.b_shift_step, b_clen=g.b_clen, b_relu=g.b_relu, b_index_zstride=g.b_index_zstride,
              b_index_mod=g.b_index_mod, ldc=g.ldc, c_zstride=g.c_zstride, ldd=g.ldd, d_zstride=g.d_zstride, lde=g.lde,
              e_zstride=g.e_zstride, relu=g.relu, accumulate=g.accumulate, nbatch=g.nbatch, ksplit=g.ksplit, kchunk=g.kchunk,
              nlayer=g.nlayer, a_lstride=g.a_lstride, b_lstride=g.b_lstride, b_dil_depth=g.b_dil_depth, b_layer0=g.b_layer0)
    if device == "cpu" and c.fence:
        # host only: the emulator reads A where it ends at an inaccessible page.  On a GPU the operand is the guarded tensor
        # above, so that an over-read there stays inside the allocation.
        assert g.a_off == 0
        dev["A"], start, mapping = _fenced(c.A)
        c.tA = dev["A"].clone()
        kw["A"] = dev["A"].data_ptr() + 4 * start
    else:
        kw["A"] = ptr("A", c.tA, c.sA)
    kw["B"] = ptr("B", c.tB, c.sB)
    assert kw["A"] % 16 == 4 * g.a_off and kw["B"] % 16 == 4 * g.b_off
    kw["b_index"] = ptr("I", c.tI, c.sI) or None
    kw["bias"] = ptr("bias", c.tbias, c.sbias) or None
    kw["E"] = ptr("E", c.tE, c.sE) or None
    kw["C"] = ptr("C", c.tC, c.sC)
    kw["D"] = kw["C"] if g.d_in_place else (ptr("D", c.tD, c.sD) or None)
    kw["a_rowsum"] = ptr("R", c.tR, c.sR if c.tR is not None else 0) or None
    run_gemm(lib, device, **kw)

    what = "%s/%s" % (c.name, data)
    # the inputs are unchanged (in place, D is C)
    for name, t in (("A", c.tA), ("B", c.tB), ("I", c.tI), ("bias", c.tbias), ("D", c.tD), ("E", c.tE)):
        if t is not None:
            view = torch.int64 if t.dtype == torch.int64 else torch.int32
            assert torch.equal(dev[name].cpu().view(view), t.view(view)), (what, name, "input changed")
    outC = dev["C"].cpu()
    got = outC[c.c_idx]
    rest = torch.ones(outC.numel(), dtype=torch.bool)
    rest[c.c_idx.reshape(-1)] = False
    assert bool((outC.view(torch.int32)[rest] == SENTINEL).all()), (what, "a store outside C")
    ratio = 0.0
    if data == "exact":
        want = torch.from_numpy(c.ref).float()
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            z, m, n = (int(v) for v in bad[0])
            raise AssertionError("%s: %d elements differ, first C[z=%d][m=%d][n=%d] = %r, want %r" %
                                 (what, bad.shape[0], z, m, n, float(got[z, m, n]), float(want[z, m, n])))
    else:
        err = (got.double() - torch.from_numpy(c.ref)).abs()
        bound = torch.from_numpy((c.kz[:, None, None] + 4) * U * c.mag)
        assert bool(torch.isfinite(got).all()), (what, "non-finite result")
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= bound).all()), (what, "error / bound", ratio)
    if c.tR is not None:
        outR = dev["R"].cpu()
        gotR = outR[c.sR:c.sR + g.nz * g.M].reshape(g.nz, g.M)
        restR = torch.ones(outR.numel(), dtype=torch.bool)
        restR[c.sR:c.sR + g.nz * g.M] = False
        assert bool((outR.view(torch.int32)[restR] == SENTINEL).all()), (what, "a store outside a_rowsum")
        if data == "exact":
            assert torch.equal(gotR, torch.from_numpy(c.ref_rows).float()), (what, "a_rowsum")
        else:
            errR = (gotR.double() - torch.from_numpy(c.ref_rows)).abs()
            boundR = torch.from_numpy((c.kz[:, None] + 4) * U * c.rows_mag)
            assert bool((errR <= boundR).all()), (what, "a_rowsum", float((errR / boundR.clamp_min(1e-300)).max()))
            ratio = max(ratio, float((errR / boundR.clamp_min(1e-300)).max()))
    return ratio


# ------------------------------------------------------------------------------------------------------------------
# path predictor: the kernel's block-uniform decisions, restated per block and k-tile
# ------------------------------------------------------------------------------------------------------------------
A_FWD = ["a_vec", "a_scalar:ragged_m", "a_scalar:lda", "a_scalar:misaligned"]
B_FWD = ["b_vec", "b_scalar:shift_mod4", "b_scalar:left_edge", "b_scalar:right_edge", "b_scalar:ldb", "b_scalar:seg_stride",
         "b_scalar:misaligned", "b_scalar:ragged_n", "b_unaligned_seg:seg_len", "b_unaligned_seg:kbeg", "b_mixed"]
A_DW = ["a_kvec", "a_kscalar:ragged_m", "a_kscalar:kchunk_mod4", "a_kscalar:lda", "a_kscalar:misaligned"]
B_DW = ["b_kvec", "b_kscalar:left_edge", "b_kscalar:right_edge", "b_kscalar:partial_tile", "b_kscalar:shift_mod4",
        "b_kscalar:row_offset_mod4", "b_kscalar:ragged_n", "b_kmixed"]
OTHER = ["k_tail", "k_lt_32", "k_zero", "multi_seg_tile_rows", "shift_ge_n", "neg_shift", "dilated_layers"]
EPILOGUE = ["bias", "D", "E", "relu", "accumulate", "b_relu", "a_rowsum", "d_in_place"]
VARIANTS = ["variant(%d,%d,%d,%d)" % (tm, tn, km, oh) for tm in (1, 2) for tn in (1, 2) for km, oh in ((0, 0), (1, 0), (1, 1))]
ALL_LABELS = set(A_FWD + B_FWD + A_DW + B_DW + OTHER + EPILOGUE + VARIANTS)


def _why(labels, prefix, failing):
    """a scalar path is labelled by its cause only where that cause stands alone: dropping that one test from the kernel's
    predicate would then change the path"""
    bad = [k for k, v in failing.items() if v]
    if len(bad) == 1:
        labels.add(prefix + bad[0])


def predict_paths(g):
    """Labels of everything a launch with these arguments exercises (the operand bases are 16-byte aligned + a_off / b_off floats)."""
    L = set()
    kmaj, onehot = g.a_kmajor, bool(g.onehot)
    tm, tn = (2 if g.M > 64 else 1), (2 if g.N > 64 else 1)
    BM, BN = 64 * tm, 64 * tn
    L.add("variant(%d,%d,%d,%d)" % (tm, tn, kmaj, int(onehot)))
    for name, on in (("bias", g.has_bias), ("D", g.has_D), ("E", g.has_E), ("relu", g.relu), ("accumulate", g.accumulate),
                     ("b_relu", g.b_relu), ("a_rowsum", g.has_rowsum), ("d_in_place", g.d_in_place)):
        if on:
            L.add(name)
    rows = g.N if kmaj else g.K
    one_seg = g.b_seg_len >= rows
    nseg = 1 if one_seg else -(-rows // g.b_seg_len)
    axis = g.K if kmaj else g.N                      # length of the contiguous axis the shifts move along
    for li in range(g.nlayer):
        dmul = 1 << ((g.b_layer0 + li) % g.b_dil_depth) if g.b_dil_depth > 0 else 1
        sh0, shstep = g.b_shift0 * dmul, g.b_shift_step * dmul
        shifts = [sh0 + s * shstep for s in range(nseg)]
        if any(s >= axis for s in shifts) and axis > 0:
            L.add("shift_ge_n")
        if any(s < 0 for s in shifts):
            L.add("neg_shift")
        if g.nlayer > 1 and g.b_dil_depth > 0 and dmul > 1 and any(shifts):
            L.add("dilated_layers")
        for b in range(g.nbatch):
            a_aligned = (g.a_off + li * g.a_lstride + b * g.a_zstride) % 4 == 0
            b_aligned = (g.b_off + li * g.b_lstride + b * g.b_zstride) % 4 == 0
            for ks in range(g.ksplit):
                kbeg = ks * g.kchunk
                kend = kbeg + g.kchunk if g.K - kbeg > g.kchunk else g.K
                klen = max(0, kend - kbeg)
                nk = -(-klen // WN_BK)
                if klen == 0:
                    L.add("k_zero")
                    continue
                if klen < WN_BK:
                    L.add("k_lt_32")
                elif klen % WN_BK:
                    L.add("k_tail")
                tiles = [kbeg + t * WN_BK for t in range(nk)]
                for m0 in range(0, g.M, BM):
                    for n0 in range(0, g.N, BN):
                        if kmaj:
                            _predict_dw(L, g, onehot, one_seg, sh0, shstep, kbeg, kend, tiles, m0, n0, BM, BN, a_aligned, b_aligned)
                        else:
                            _predict_fwd(L, g, one_seg, sh0, shstep, kbeg, tiles, m0, n0, BM, BN, a_aligned, b_aligned)
    return L


def _predict_fwd(L, g, one_seg, sh0, shstep, kbeg, tiles, m0, n0, BM, BN, a_aligned, b_aligned):
    a_fail = {"ragged_m": m0 + BM > g.M, "lda": g.lda % 4 != 0, "misaligned": not a_aligned}
    if any(a_fail.values()):
        _why(L, "a_scalar:", a_fail)
    else:
        L.add("a_vec")
    if not one_seg and g.b_seg_len % WN_BK != 0:
        L.add("b_unaligned_seg:seg_len")
        return
    if not one_seg and kbeg % WN_BK != 0:
        L.add("b_unaligned_seg:kbeg")
        return
    static = {"ldb": g.ldb % 4 != 0, "seg_stride": g.b_seg_stride % 4 != 0, "ragged_n": n0 + BN > g.N, "misaligned": not b_aligned}
    kinds = set()
    for k0 in tiles:
        seg = 0 if one_seg else k0 // g.b_seg_len
        cc0 = n0 - (sh0 + seg * shstep)
        fail = dict(static)
        fail.update({"shift_mod4": cc0 % 4 != 0, "left_edge": cc0 < 0, "right_edge": cc0 + BN > g.b_clen})
        if any(fail.values()):
            _why(L, "b_scalar:", fail)
            kinds.add("scalar")
        else:
            L.add("b_vec")
            kinds.add("vec")
    if len(kinds) == 2:
        L.add("b_mixed")


def _predict_dw(L, g, onehot, one_seg, sh0, shstep, kbeg, kend, tiles, m0, n0, BM, BN, a_aligned, b_aligned):
    if not one_seg and n0 // g.b_seg_len != (min(n0 + BN, g.N) - 1) // g.b_seg_len:
        L.add("multi_seg_tile_rows")
    if onehot:
        return                                        # every load of the one-hot variants is scalar
    k_base_bad = kbeg % 4 != 0 or kend % 4 != 0
    a_fail = {"ragged_m": m0 + BM > g.M, "kchunk_mod4": k_base_bad, "lda": g.lda % 4 != 0, "misaligned": not a_aligned}
    if any(a_fail.values()):
        _why(L, "a_kscalar:", a_fail)
    else:
        L.add("a_kvec")
    # the row table: every row of the tile, the ones past N too (they take part in the shift test, not in the offset test)
    sh_bad = off_bad = False
    for n in range(n0, n0 + BN):
        seg, rr = (0, n) if one_seg else (n // g.b_seg_len, n % g.b_seg_len)
        if (sh0 + seg * shstep) % 4 != 0:
            sh_bad = True
        if n < g.N and (seg * g.b_seg_stride + rr * g.ldb) % 4 != 0:
            off_bad = True
    shmin = shmax = sh0
    if not one_seg:
        s_lo, s_hi = sh0 + (n0 // g.b_seg_len) * shstep, sh0 + ((n0 + BN - 1) // g.b_seg_len) * shstep
        shmin, shmax = min(s_lo, s_hi), max(s_lo, s_hi)
    static = {"kchunk_mod4": k_base_bad, "shift_mod4": sh_bad, "row_offset_mod4": off_bad, "ragged_n": n0 + BN > g.N,
              "misaligned": not b_aligned}
    kinds = set()
    for k0 in tiles:
        fail = dict(static)
        fail.update({"left_edge": k0 - shmax < 0, "right_edge": k0 + WN_BK - shmin > g.b_clen, "partial_tile": k0 + WN_BK > kend})
        if any(fail.values()):
            bad = [k for k, v in fail.items() if v]
            if len(bad) == 1 and "b_kscalar:" + bad[0] in ALL_LABELS:
                L.add("b_kscalar:" + bad[0])
            kinds.add("scalar")
        else:
            L.add("b_kvec")
            kinds.add("vec")
    if len(kinds) == 2:
        L.add("b_kmixed")


# ------------------------------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------------------------------
def _case(name, **kw):
    kw["name"] = name
    return kw


# fmaxf(NaN, 0) = 0: in a case with `relu` or `b_relu` a guard-band over-read comes out as 0, not NaN, and shows only where the
# right value is not 0.  Such cases are here for the epilogue / b_relu labels; no staging-path label may hang on one of them alone.
CASES = [
    # ---- forward / dX type ---------------------------------------------------------------------------------------
    _case("f_plain_128", M=128, N=128, K=96, bias=1),
    _case("f_64_relu", M=64, N=64, K=128, relu=1, nbatch=2, a_zstride=0),
    _case("f_ragged_n_130_k24", M=64, N=130, K=24, bias=1),
    # vector-eligible with K % 32 != 0: the rows past K of the LAST batch of the LAST layer are guard band
    _case("f_ktail_vec_last_batch", M=130, N=64, K=100, nbatch=2, nlayer=2),
    _case("f_taps_4_0_n256", M=128, N=256, K=128, seg_len=64, shift0=4, shift_step=-4, bias=1),
    _case("f_taps_8_4_0_n384", M=64, N=384, K=96, seg_len=32, shift0=8, shift_step=-4),
    _case("f_shift_1_0", M=64, N=256, K=128, seg_len=64, shift0=1, shift_step=-1),
    _case("f_shift_3_2_1", M=33, N=200, K=96, seg_len=32, shift0=3, shift_step=-1),
    _case("f_clen_lt_n", M=64, N=256, K=96, clen=200),
    _case("f_clen_gt_n", M=64, N=130, K=96, clen=256),
    _case("f_clen_lt_n_shifted", M=65, N=200, K=128, seg_len=64, clen=130, shift0=16, shift_step=-16, nbatch=2),
    _case("f_shift_ge_n", M=64, N=65, K=128, seg_len=64, shift0=80, shift_step=-80, bias=1),
    _case("f_neg_shift_dx_taps", M=128, N=256, K=96, seg_len=32, shift0=-8, shift_step=4),
    _case("f_neg_shift_odd", M=33, N=130, K=128, seg_len=64, shift0=-3, shift_step=3, b_relu=1),
    _case("f_seg12", M=65, N=130, K=100, seg_len=12, shift0=8, shift_step=-1),
    _case("f_seg80_aux", M=128, N=128, K=160, seg_len=80, shift0=2, shift_step=-2, bias=1),
    _case("f_seg64_partial_last", M=64, N=128, K=160, seg_len=64, shift0=8, shift_step=-4),
    _case("f_seg_stride_mod4", M=128, N=128, K=128, seg_len=64, seg_stride=64 * 128 + 8),
    _case("f_seg_stride_odd", M=128, N=128, K=128, seg_len=64, seg_stride=64 * 128 + 3),
    _case("f_ksplit3_kchunk32", M=128, N=65, K=96, ksplit=3, kchunk=32, accumulate=1),
    _case("f_ksplit3_kchunk40", M=64, N=128, K=100, ksplit=3, kchunk=40, nbatch=2),
    _case("f_ksplit3_kchunk40_seg64", M=64, N=128, K=100, seg_len=64, ksplit=3, kchunk=40, shift0=4, shift_step=-4),
    _case("f_layers3_dil_D", M=130, N=128, K=128, seg_len=64, shift0=4, shift_step=-4, nlayer=3, nbatch=2, dil_depth=2,
          layer0=1, D=1, bias=1),
    _case("f_layers2_layer0", M=64, N=64, K=24, seg_len=12, shift0=1, shift_step=-1, nlayer=2, dil_depth=3, layer0=2, a_zstride=0,
          nbatch=2),
    _case("f_a_misaligned", M=128, N=128, K=96, a_off=1),
    _case("f_b_misaligned", M=128, N=128, K=96, b_off=2),
    _case("f_lda_odd", M=128, N=128, K=96, lda=129),
    _case("f_ldb_odd", M=128, N=128, K=96, ldb=129),
    _case("f_zstride_odd", M=64, N=64, K=7, nbatch=3, a_zstride=7 * 64 + 1, b_zstride=7 * 64 + 2),
    _case("f_k0_epilogue_only", M=65, N=33, K=0, bias=1, D=1, accumulate=1),
    _case("f_1x1_k7", M=1, N=1, K=7, bias=1),
    _case("f_d_in_place", M=128, N=130, K=96, d_in_place=1, relu=1, nbatch=2, ldc=133),
    _case("f_full_epilogue", M=200, N=200, K=96, bias=1, D=1, E=1, relu=1, accumulate=1, ldc=203),
    _case("f_mask_accumulate", M=33, N=65, K=24, E=1, accumulate=1, nbatch=2),
    _case("f_b_relu", M=64, N=130, K=100, b_relu=1),
    _case("f_384_nbatch3", M=384, N=384, K=160, nbatch=3, bias=1, a_zstride=0),
    # ---- dW type (k = time) -----------------------------------------------------------------------------------------
    _case("w_plain_64", mode="dw", M=64, N=64, K=256, ksplit=2, kchunk=128, rowsum=1),
    _case("w_taps_4_0", mode="dw", M=128, N=128, K=320, seg_len=64, shift0=4, shift_step=-4, rowsum=1),
    _case("w_first_last_scalar", mode="dw", M=128, N=128, K=320, seg_len=64, shift0=4, shift_step=-8, nbatch=2),
    _case("w_neg_shift", mode="dw", M=64, N=128, K=256, seg_len=64, shift0=-4, shift_step=4),
    _case("w_shift_1_0", mode="dw", M=128, N=128, K=256, seg_len=64, shift0=1, shift_step=-1),
    _case("w_ldb_odd", mode="dw", M=64, N=64, K=128, ldb=129),
    _case("w_ragged_130", mode="dw", M=130, N=130, K=128, rowsum=1),
    # A ends at an inaccessible page (host): rows M .. BM of a 16-byte A load would be read from there
    _case("w_ragged_m_65_fenced", mode="dw", M=65, N=64, K=128, fence_a=1, rowsum=1),
    _case("w_33x130", mode="dw", M=33, N=130, K=100, b_relu=1, bias=1),
    _case("w_130x33", mode="dw", M=130, N=33, K=24, accumulate=1),
    _case("w_kchunk_mod4", mode="dw", M=64, N=64, K=300, ksplit=3, kchunk=102, rowsum=1),
    _case("w_kchunk40_partial", mode="dw", M=64, N=64, K=160, ksplit=4, kchunk=40, rowsum=1),
    _case("w_lda_odd", mode="dw", M=64, N=64, K=128, lda=129),
    _case("w_a_misaligned", mode="dw", M=64, N=64, K=128, a_off=3),
    _case("w_b_misaligned", mode="dw", M=64, N=64, K=128, b_off=1),
    _case("w_layers3_ksplit2_rowsum", mode="dw", M=65, N=128, K=128, seg_len=64, shift0=2, shift_step=-2, nlayer=3, nbatch=2,
          ksplit=2, kchunk=64, rowsum=1, dil_depth=3, layer0=2),
    _case("w_clen_lt_k", mode="dw", M=64, N=64, K=256, clen=200),
    _case("w_seg_stride", mode="dw", M=64, N=200, K=700, seg_len=100, seg_stride=100 * 700 + 4, shift0=8, shift_step=-8, ksplit=2,
          kchunk=352),
    _case("w_k0", mode="dw", M=33, N=33, K=0, rowsum=1, bias=1),
    _case("w_onehot_33x64", mode="dw", M=33, N=64, K=100, onehot=32, shift0=1, shift_step=-1, rowsum=1),
    _case("w_onehot_130x37", mode="dw", M=130, N=37, K=96, onehot=37, nbatch=2),
    _case("w_onehot_64x74", mode="dw", M=64, N=74, K=300, onehot=37, shift0=1, shift_step=-1, ksplit=3, kchunk=128, nbatch=2),
    _case("w_onehot_130x200", mode="dw", M=130, N=200, K=160, onehot=100, shift0=2, shift_step=-2, rowsum=1),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
CASE_NAMES = [c["name"] for c in CASES]


def coverage():
    """label -> names of the cases that exercise it"""
    cov = {}
    for c in CASES:
        for lab in predict_paths(make_args(c)):
            cov.setdefault(lab, []).append(c["name"])
    return cov
