"""-m gpu: attention at the boundary the header documents -- independent strided views, tile edges, grouped kv heads, hard softmax inputs.

A. `_call` drives gaot_attention_fwd_ws / _bwd (and the two _dropout entries, with the two _workspace queries) through ctypes on views
   carved out of ONE device allocation: every tensor (q, k, v, o, lse, dout, dq, dk, dv, both workspaces) sits between guard bands of
   4 096 floats, with its own base offset, row pitch and used columns.  Guard bands, pitch padding and every output element hold a finite
   sentinel before the call; after it everything outside the output regions is bit-identical to what it was (inputs included), every
   output element is finite and no longer the sentinel, and o, lse, dq, dk, dv match float64 tensor by tensor.

   Alignment guards, read in gaot_attention_fwd_ws / gaot_attention_bwd and the kernels they launch before the first run (each is now
   a boolean of AttnFacts in csrc/attention_plan.h -- vec, o_aligned, ldo4, ws_aligned, dq_ / dk_ / dv_aligned, lddq4 / lddk4 / lddv4,
   dq_part_aligned -- gathered in one place, attention.hip gather_facts, and read by plan_attention):
     * q / k / v loads: 16-byte loads only behind AttnArgs.vec (head_dim, ldq, ldk, ldv multiples of 4, q, k, v 16-byte aligned); the
       backward adds ldo % 4 and aligned16(dout) to it (the 16-byte dO loads).                                             guarded
     * stores to o (every forward kernel), to dk / dv (every backward kernel), to dq of the wide kernels: scalar.          guarded
     * attn_fwd_combine_kernel (16-byte stores to o): behind aligned16(o), ldo % 4, aligned16(workspace).                  guarded
     * attn_delta_vec_kernel, the fused delta of the fp16 8-wave kernels (16-byte loads of o): behind vec && aligned16(o). guarded
     * attn_dq_reduce_vec_kernel: stores behind aligned16(dq) && lddq % 4; its 16-byte loads of the dQ slabs, which start B*H*S floats
       into the workspace, were behind nothing (S = 33, H = 1: a 4-byte aligned slab).                                     FIXED
     * attn_add_cols_kernel (query-split backward, head_dim 32 and 33..64): 16-byte read-modify-writes at dk + r * lddk, dv + r * lddv
       behind aligned16(dk / dv) but neither lddk % 4 nor lddv % 4, and 16-byte loads of the second half's partials, which
       sit behind the dQ slabs.                                                                                            FIXED
   The fixes add `lddk % 4 == 0 && lddv % 4 == 0 && aligned16(dq_part)` to the two query-split conditions and `aligned16(dq_part)` to
   the vector dQ reduce: such calls fall back to the one-workgroup-per-key-block kernels / the scalar reduce, which compute the same
   sums in the same order.  No layout is rejected.  (gfx950 serves a misaligned 16-byte global access, so none of these showed as a
   fault or a wrong number; the dispatch now states what the kernels assume.  "only dk pitched +1" at 4 x 1 024 x 8 is the case that
   walks the fixed conditions.)  By layout: fused, separate-dense, pitched+4, pitched+1, offset+1, only o / dout / dq offset and only
   ldo + 1 were found guarded by reading; only dk pitched + 1 (and any layout with B*H*S no multiple of 4) needed the fix.

   A magnitude word is GAOT_AMAX_SLOTS * GAOT_AMAX_STRIDE = 1 024 floats (include/gaot_hip.h), not one float: the words here are zeroed
   1 024-float tensors with max |x| (computed on the host) in slot 0.

B. grouped kv heads (H / Hkv = 4, 8): dk / dv arrive as one block per QUERY head; lse against logsumexp in float64 in every harness case.
C. S = 1 .. 257 around the 32 / 64 / 128 / 256 tile edges; the wide kernels at B*H = 8, 16, 24 (the XCD branch of xcd_group_decode).
D. hard inputs per path, out, dq, dk, dv each against its own float64 block, bar = max(project bar, 4 x the error of the same closed
   form in float32 on the CPU).  Measured (kernel error / float32-reference error, worst tensor of out, dq, dk, dv by ratio):

   path        | peaked                      | qk+1                        | v+30                        | qkx3                        | vx30                        | dout*1e-6
   D32         | dv 2.6e-06 / 2.6e-07 = 10.0 | o  4.5e-07 / 7.6e-07 =  0.6 | dq 5.7e-06 / 4.4e-06 =  1.3 | dq 2.4e-06 / 1.3e-06 =  1.8 | o  2.0e-07 / 3.4e-07 =  0.6 | o  2.0e-07 / 3.4e-07 =  0.6
   D32-bf16x3  | dv 2.6e-06 / 2.6e-07 =  9.8 | o  5.3e-07 / 7.6e-07 =  0.7 | dq 6.2e-06 / 4.4e-06 =  1.4 | dv 1.6e-06 / 6.9e-07 =  2.3 | o  2.1e-07 / 3.4e-07 =  0.6 | o  2.1e-07 / 3.4e-07 =  0.6
   D32-split0  | dv 2.6e-06 / 2.1e-07 = 12.5 | o  7.6e-07 / 7.6e-07 =  1.0 | dq 1.2e-05 / 4.4e-06 =  2.7 | o  6.4e-07 / 7.0e-07 =  0.9 | o  3.2e-07 / 3.4e-07 =  0.9 | o  3.2e-07 / 3.4e-07 =  1.0
   D48         | dq 1.2e-06 / 8.3e-07 =  1.4 | o  5.8e-07 / 1.0e-06 =  0.6 | dq 6.5e-06 / 4.9e-06 =  1.3 | dq 1.5e-06 / 1.7e-06 =  0.9 | o  2.1e-07 / 3.3e-07 =  0.6 | o  2.1e-07 / 3.3e-07 =  0.6
   D64-split2  | dv 3.8e-06 / 2.7e-07 = 14.3 | o  7.8e-07 / 1.3e-06 =  0.6 | dq 5.5e-06 / 4.9e-06 =  1.1 | o  6.2e-07 / 9.0e-07 =  0.7 | o  2.1e-07 / 3.9e-07 =  0.6 | o  2.2e-07 / 3.5e-07 =  0.6
   D96         | dv 4.5e-06 / 3.1e-07 = 14.8 | o  1.7e-06 / 1.7e-06 =  1.0 | dq 9.8e-06 / 5.8e-06 =  1.7 | o  1.0e-06 / 1.0e-06 =  1.0 | o  4.0e-07 / 4.0e-07 =  1.0 | o  4.0e-07 / 4.0e-07 =  1.0
   D128        | dv 5.4e-06 / 3.1e-07 = 17.2 | o  2.3e-06 / 2.3e-06 =  1.0 | dq 9.6e-06 / 6.4e-06 =  1.5 | dk 2.9e-06 / 2.4e-06 =  1.2 | o  4.6e-07 / 4.6e-07 =  1.0 | o  4.6e-07 / 4.6e-07 =  1.0
   D192        | dv 3.9e-06 / 3.7e-07 = 10.5 | dq 1.4e-06 / 2.8e-06 =  0.5 | dq 9.0e-06 / 7.7e-06 =  1.2 | dk 1.6e-06 / 2.9e-06 =  0.6 | o  3.3e-07 / 5.2e-07 =  0.6 | o  3.3e-07 / 5.2e-07 =  0.6
   D256        | dv 6.7e-06 / 3.1e-07 = 21.8 | dv 1.6e-06 / 2.2e-06 =  0.8 | dq 9.2e-06 / 6.8e-06 =  1.4 | dq 1.7e-06 / 1.9e-06 =  0.9 | o  3.1e-07 / 3.8e-07 =  0.8 | o  3.1e-07 / 3.8e-07 =  0.8

   (B = 1, S = 160, H = 2, the worse of Hkv = 2 and 1; the tensor shown is the one closest to its bar.)  Every case passes; the closest is
   0.67 of its bar (dv of the peaked input at head_dim 256).  Two things the table shows:
     * v x 30 beside unit q, k under ONE magnitude word costs the fp16-piece kernels nothing (ratio 0.6, as bf16x3): no second word needed;
     * the peaked input's dv sits 10 .. 22 x above the float32 closed form on EVERY path, the fp32-MFMA kernels included, still under the
       project bar of 1e-5: the backward recomputes P = exp2(s c - lse) at |s c| of several hundred (54 sqrt(head_dim) log2 e) where the closed form keeps the forward's P, so
       the rounding of the score itself (2^-24 |s c|) enters P.  It is a property of the recomputation, not of a kernel.

   S = 1 (softmax == 1): `out == v` bit for bit, dq and dk zero to the bar, dv exact.  The tiled forward kernels reached out = v only to
   one or two units in the last place on five cases (found by this module):
     * head_dim 32 and 64, default and split 2 (the fp16-piece kernels): v passes through two fp16 pieces, 22 of its 24 bits
       (common.h split2h_pair: "up to the operand's last bit") -- max |out - v| 2.4e-7 (2 ulp) at 32, 1.2e-7 (1 ulp) at 64;
     * head_dim 32, split 0 (attn_fwd_glds_kernel): the exponent is formed as fma(s, c, -rn(m c)), the rounding residual of m c and
       not zero at the maximum, so P = 1 - 2^-24 where it should be 1 and out = rn(rn(P v) / P) -- max |out - v| 1.2e-7 (1 ulp).
   Changing the exponent form or adding a piece would move every output of those kernels, so gaot_attention_fwd_ws now answers a single
   key with attn_fwd_one_key_kernel (out = v copied, lse = scale <q, k>) for every head_dim and `pieces`; the S = 1 forward cases here
   therefore run that kernel whatever the split switch says, the backward cases the tiled kernels.
"""
import contextlib
import ctypes as C
import functools
import math

import pytest
import torch

from tests.test_ops_gpu import _dropout_factor, dev

pytestmark = pytest.mark.gpu

GUARD = 4096                  # floats before and after every tensor
SENTINEL = -1234.5678         # finite, far from anything the data produces
WORD = 32 * 32                # floats per magnitude word (GAOT_AMAX_SLOTS * GAOT_AMAX_STRIDE)
BAR_OUT, BAR_GRAD = 3e-6, 1e-5          # the project's bars for these kernels, rel-L2 against float64 on randn


def _rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


@contextlib.contextmanager
def _switches(**kw):
    """gaot_debug_set_attention_<name>(value) for the block, every one restored afterwards"""
    from gaot_amd import _lib
    lib, old = _lib.load(), []
    try:
        for name, val in kw.items():
            fn = getattr(lib, f"gaot_debug_set_attention_{name}")
            old.append((fn, fn(int(val))))
        yield
    finally:
        for fn, val in reversed(old):
            fn(val)


@contextlib.contextmanager
def _f32_pieces(name):
    from gaot_amd import ops
    old = ops.set_f32_pieces(name)
    try:
        yield
    finally:
        ops.set_f32_pieces(old)


# ------------------------------------------------------------------------------------------------------------------
# references: the closed form by autograd, in the dtype asked for, with dK / dV per QUERY head
# ------------------------------------------------------------------------------------------------------------------
def _closed_form(q, k, v, go, dtype, fac=None):
    """q, go [B,S,H,D], k, v [B,S,Hkv,D] -> out [B,S,H,D], lse [B,H,S], dq, dk, dv [B,S,H,D] (dk, dv per query head)"""
    H, Hkv, D = q.shape[2], k.shape[2], q.shape[3]
    r = H // Hkv
    qh = q.to(dtype).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    kh = k.to(dtype).repeat_interleave(r, dim=2).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    vh = v.to(dtype).repeat_interleave(r, dim=2).permute(0, 2, 1, 3).contiguous().requires_grad_(True)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(D)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    if fac is not None:
        p = p * fac.to(dtype)
    out = p @ vh
    out.backward(go.to(dtype).permute(0, 2, 1, 3))
    back = lambda t: t.detach().permute(0, 2, 1, 3).contiguous()
    return dict(o=back(out), lse=lse.detach(), dq=back(qh.grad), dk=back(kh.grad), dv=back(vh.grad))


def _group_sum(t, Hkv):
    B, S, H, D = t.shape
    return t.reshape(B, S, Hkv, H // Hkv, D).sum(3)


def _randn_case(B, S, H, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, H, D, generator=g), torch.randn(B, S, Hkv, D, generator=g), torch.randn(B, S, Hkv, D, generator=g),
            torch.randn(B, S, H, D, generator=g))


@functools.lru_cache(maxsize=None)
def _case(B, S, H, Hkv, D, seed=0, p_drop=0.0, drop_seed=0):
    """seeded randn inputs with their float64 and float32 references: computed once, shared, never modified"""
    q, k, v, go = _randn_case(B, S, H, Hkv, D, 1000 * seed + 7 * S + D + H)
    fac = _dropout_factor(drop_seed, B, H, S, p_drop) if p_drop > 0.0 else None
    return (q, k, v, go), _closed_form(q, k, v, go, torch.float64, fac), _closed_form(q, k, v, go, torch.float32, fac)


# ------------------------------------------------------------------------------------------------------------------
# A. the harness
# ------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("fused", "separate-dense", "pitched+4", "pitched+1", "offset+1",
           "only-o-offset", "only-dout-offset", "only-dq-offset", "only-dk-pitch+1", "only-ldo+1")
_TENSORS = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")


def _layout(name, H, Hkv, D):
    """per tensor (used columns, pitch padding, base shift in floats); `fused` is handled by _Arena.fused"""
    cols = dict(q=H * D, k=Hkv * D, v=Hkv * D, o=H * D, dout=H * D, dq=H * D, dk=H * D, dv=H * D)
    pad, shift = dict.fromkeys(_TENSORS, 0), dict.fromkeys(_TENSORS, 0)
    if name == "pitched+4":
        pad = dict.fromkeys(_TENSORS, 4)
    elif name == "pitched+1":
        pad = dict.fromkeys(_TENSORS, 1)
    elif name == "offset+1":
        shift = dict.fromkeys(_TENSORS, 1)
    elif name == "only-o-offset":
        shift["o"] = 1
    elif name == "only-dout-offset":
        shift["dout"] = 1
    elif name == "only-dq-offset":
        shift["dq"] = 1
    elif name == "only-dk-pitch+1":
        pad["dk"] = 1
    elif name == "only-ldo+1":               # o and dout share ldo in gaot_attention_bwd
        pad["o"] = pad["dout"] = 1
    else:
        assert name in ("fused", "separate-dense"), name
    return cols, pad, shift


class _Arena:
    """one allocation; every region between guard bands; views = (base, rows, cols, pitch) in floats"""

    def __init__(self):
        self.cur, self.views, self.outputs, self.scratch = 0, {}, [], []

    def region(self, rows, pitch, shift=0):
        base = (self.cur + GUARD + 3) // 4 * 4 + shift           # 16-byte aligned, then the layout's shift
        self.cur = base + rows * pitch
        return base

    def add(self, name, rows, cols, pad=0, shift=0, output=False):
        self.views[name] = (self.region(rows, cols + pad, shift), rows, cols, cols + pad)
        if output:
            self.outputs.append(name)

    def alias(self, name, of_base, col0, rows, cols, pitch, output=False):
        self.views[name] = (of_base + col0, rows, cols, pitch)
        if output:
            self.outputs.append(name)

    def work(self, name, n):
        self.views[name] = (self.region(1, max(n, 4)), 1, n, max(n, 4))
        self.scratch.append(name)

    def total(self):
        return self.cur + GUARD

    def strided(self, flat, name):
        base, rows, cols, pitch = self.views[name]
        return flat.as_strided((rows, cols), (pitch, 1), base)


def _word(value):
    w = torch.zeros(WORD)
    w[0] = float(value)
    return w.to(dev())


def _call(layout, q, k, v, go, pieces=3, p_drop=0.0, drop_seed=0):
    """forward then backward through the C entry points on the layout's views; returns o, lse, dq, dk, dv (CPU, dk / dv per query head)
    and, with pieces = 4, the published dq|dk|dv magnitude.  Asserts the canaries."""
    from gaot_amd import _lib
    from gaot_amd.ops import _stream
    lib = _lib.load()
    B, S, H, D = q.shape
    Hkv, M = k.shape[2], B * S
    cols, pad, shift = _layout(layout, H, Hkv, D)
    ar = _Arena()
    if layout == "fused":              # what ops.attention passes for Hkv < H: q|k|v one buffer, dq inside a dqkv buffer, dk / dv dense per query head
        W = (H + 2 * Hkv) * D
        qkv = ar.region(M, W)
        ar.alias("q", qkv, 0, M, H * D, W)
        ar.alias("k", qkv, H * D, M, Hkv * D, W)
        ar.alias("v", qkv, (H + Hkv) * D, M, Hkv * D, W)
        dqkv = ar.region(M, W)
        ar.alias("dq", dqkv, 0, M, H * D, W, output=True)       # (the k|v columns of dqkv stay sentinel: canary beside every dq row)
        for n in ("o", "dout", "dk", "dv"):
            ar.add(n, M, cols[n], output=n != "dout")
    else:
        for n in _TENSORS:
            ar.add(n, M, cols[n], pad[n], shift[n], output=n in ("o", "dq", "dk", "dv"))
    ar.add("lse", 1, B * H * S, output=True)
    n_wf = int(lib.gaot_attention_fwd_workspace(B, S, H, D)) if p_drop == 0.0 else 0
    n_wb = int(lib.gaot_attention_bwd_workspace(B, S, H, D))
    assert n_wf >= 0 and n_wb >= B * H * S
    ar.work("wsf", n_wf)
    ar.work("wsb", n_wb)

    img = torch.full((ar.total(),), SENTINEL, dtype=torch.float32)
    for n, t in (("q", q), ("k", k), ("v", v), ("dout", go)):
        ar.strided(img, n).copy_(t.reshape(M, -1))
    may_change = torch.zeros(ar.total(), dtype=torch.bool)
    for n in ar.outputs + ar.scratch:
        ar.strided(may_change, n).fill_(True)
    buf = img.to(dev())
    ptr = lambda n: C.c_void_p(buf.data_ptr() + 4 * ar.views[n][0])
    ld = lambda n: ar.views[n][3]
    assert ld("o") == ld("dout")

    qw = gw = dw = None
    if pieces == 4:
        qw = _word(max(float(q.abs().max()), float(k.abs().max()), float(v.abs().max())))
        gw = _word(float(go.abs().max()))
        dw = _word(0.0)
    wp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    if p_drop > 0.0:
        seed = torch.tensor([drop_seed], dtype=torch.int64).to(dev())
        _lib.check(lib.gaot_attention_fwd_dropout(ptr("q"), ptr("k"), ptr("v"), ld("q"), ld("k"), ld("v"), B, S, H, Hkv, D, ptr("o"), ld("o"),
                                                  ptr("lse"), float(p_drop), wp(seed), _stream()), "gaot_attention_fwd_dropout")
        _lib.check(lib.gaot_attention_bwd_dropout(ptr("q"), ptr("k"), ptr("v"), ld("q"), ld("k"), ld("v"), ptr("o"), ptr("dout"), ld("o"),
                                                  ptr("lse"), B, S, H, Hkv, D, ptr("dq"), ptr("dk"), ptr("dv"), ld("dq"), ld("dk"), ld("dv"),
                                                  ptr("wsb"), float(p_drop), wp(seed), _stream()), "gaot_attention_bwd_dropout")
    else:
        _lib.check(lib.gaot_attention_fwd_ws(ptr("q"), ptr("k"), ptr("v"), ld("q"), ld("k"), ld("v"), B, S, H, Hkv, D, ptr("o"), ld("o"),
                                             ptr("lse"), pieces, wp(qw), ptr("wsf") if n_wf > 0 else None, _stream()), "gaot_attention_fwd_ws")
        _lib.check(lib.gaot_attention_bwd(ptr("q"), ptr("k"), ptr("v"), ld("q"), ld("k"), ld("v"), ptr("o"), ptr("dout"), ld("o"),
                                          ptr("lse"), B, S, H, Hkv, D, ptr("dq"), ptr("dk"), ptr("dv"), ld("dq"), ld("dk"), ld("dv"),
                                          ptr("wsb"), pieces, wp(qw), wp(gw), wp(dw), _stream()), "gaot_attention_bwd")
    torch.cuda.synchronize()
    after = buf.cpu()

    # 1. guard bands, pitch padding and inputs: bit-identical
    keep = ~may_change
    a_bits, b_bits = after.view(torch.int32)[keep], img.view(torch.int32)[keep]
    if not torch.equal(a_bits, b_bits):
        bad = torch.nonzero(keep)[a_bits != b_bits].flatten()
        where = []
        for off in bad[:8].tolist():
            near = min(ar.views.items(), key=lambda kv: min(abs(off - kv[1][0]), abs(off - (kv[1][0] + kv[1][1] * kv[1][3]))))
            base, rows, cols_, pitch = near[1]
            where.append(f"{near[0]}{'+' if off >= base else ''}{off - base} (row {(off - base) // pitch}, col {(off - base) % pitch} of {cols_} used, pitch {pitch})")
        raise AssertionError(f"[{layout}] {bad.numel()} floats outside the output regions were modified: " + "; ".join(where))
    # 2. every output element written and finite
    res = {}
    for n in ar.outputs:
        t = ar.strided(after, n).clone()
        assert bool(torch.isfinite(t).all()), f"[{layout}] {n}: non-finite values"
        unwritten = int((t.view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).sum())
        assert unwritten == 0, f"[{layout}] {n}: {unwritten} elements still hold the sentinel"
        res[n] = t.reshape(B, H, S) if n == "lse" else t.reshape(B, S, H, D)
    if dw is not None:
        res["word"] = float(dw.max().cpu())
    return res


def _check(tag, res, ref64, ref32, word_expected=False):
    """3. o, lse, dq, dk, dv against float64, tensor by tensor"""
    errs = {n: _rel(res[n], ref64[n]) for n in ("o", "dq", "dk", "dv")}
    e_lse = float((res["lse"].double() - ref64["lse"]).abs().max())
    e_lse32 = float((ref32["lse"].double() - ref64["lse"]).abs().max())
    print(f"[{tag}] " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()) + f"  lse {e_lse:.2e} (fp32 {e_lse32:.2e})")
    assert errs["o"] < BAR_OUT, (tag, errs)
    for n in ("dq", "dk", "dv"):
        assert errs[n] < BAR_GRAD, (tag, n, errs)
    assert e_lse <= 4 * e_lse32 + 1e-6, (tag, e_lse, e_lse32)
    if word_expected:
        top = max(float(res[n].abs().max()) for n in ("dq", "dk", "dv"))
        assert top <= res["word"] <= 4 * top, (tag, res["word"], top)


def _ops_attention(q, k, v, go, p_drop=0.0):
    """the same data through ops.attention (fused q|k|v): out, dq [B,S,H,D], dk, dv [B,S,Hkv,D] on the CPU"""
    from gaot_amd import ops
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    qkv = torch.cat([q.reshape(B, S, -1), k.reshape(B, S, -1), v.reshape(B, S, -1)], dim=-1)
    d = qkv.to(dev()).requires_grad_(True)
    out = ops.attention(d, H, Hkv, D, dropout_p=p_drop)
    out.backward(go.reshape(B, S, H * D).to(dev()))
    g = d.grad.cpu()
    return dict(o=out.detach().cpu().reshape(B, S, H, D), dq=g[..., :H * D].reshape(B, S, H, D),
                dk=g[..., H * D:(H + Hkv) * D].reshape(B, S, Hkv, D), dv=g[..., (H + Hkv) * D:].reshape(B, S, Hkv, D))


SHAPE_A = (2, 97, 4, 2)       # B, S, H, Hkv


def _layout_case(layout, D, pieces, tag, **switches):
    B, S, H, Hkv = SHAPE_A
    (q, k, v, go), ref64, ref32 = _case(B, S, H, Hkv, D)
    with _switches(**switches):
        res = _call(layout, q, k, v, go, pieces=pieces)
        if layout == "fused":       # the control: bit for bit what ops.attention computes from the same data
            with _f32_pieces("fp16x2" if pieces == 4 else "bf16x3"):
                via_ops = _ops_attention(q, k, v, go)
    _check(f"{tag} {layout} D={D} pieces={pieces}", res, ref64, ref32, word_expected=pieces == 4)
    if layout == "fused":
        assert torch.equal(res["o"], via_ops["o"]) and torch.equal(res["dq"], via_ops["dq"])
        assert torch.equal(_group_sum(res["dk"], Hkv), via_ops["dk"]) and torch.equal(_group_sum(res["dv"], Hkv), via_ops["dv"])


@pytest.mark.parametrize("pieces", [3, 4])
@pytest.mark.parametrize("D", [12, 32, 48, 64, 96, 128, 160, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(layout, D, pieces):
    _layout_case(layout, D, pieces, "layout")


@pytest.mark.parametrize("pieces", [3, 4])
def test_head_dim_255_canary_behind_the_last_column(pieces):
    _layout_case("pitched+4", 255, pieces, "layout")


# head_dim 32 .. 64 through the debug switches: 2 = the 8-wave kernels (256 queries / keys per workgroup) the heuristics pick only when they fill
# the chip, 3 = the 4-wave split kernels always, 0 = the fp32-MFMA kernels
@pytest.mark.parametrize("pieces", [3, 4])
@pytest.mark.parametrize("split", [2, 3, 0])
@pytest.mark.parametrize("D", [32, 48, 64])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_forced_kernels(layout, D, split, pieces):
    _layout_case(layout, D, pieces, f"split={split}", split=split)


@pytest.mark.parametrize("D", [32, 64, 96, 160, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts_dropout(layout, D):
    B, S, H, Hkv = SHAPE_A
    seed = 0x1234567 + D
    (q, k, v, go), ref64, ref32 = _case(B, S, H, Hkv, D, p_drop=0.25, drop_seed=seed)
    res = _call(layout, q, k, v, go, p_drop=0.25, drop_seed=seed)
    _check(f"dropout {layout} D={D}", res, ref64, ref32)


BIG_MODES = {"keysplit2": dict(keysplit=2), "split2": dict(split=2), "split2-h16-4": dict(split=2, h16=4), "split2-h16-0": dict(split=2, h16=0),
             "dh8-0": dict(dh8=0)}


@pytest.mark.parametrize("layout", ["pitched+4", "only-dk-pitch+1"])
@pytest.mark.parametrize("D,mode", [(32, "keysplit2"), (32, "split2"), (32, "split2-h16-4"), (32, "split2-h16-0"),
                                    (48, "keysplit2"), (48, "split2"), (48, "dh8-0")])
def test_layouts_query_split_and_key_split(D, mode, layout):
    """128 blocks of 256 x batch x heads: the key-split forward (head_dim 32: forced by keysplit 2) and the query-split backward with its
    attn_add_cols_kernel; with a dk pitch that is no multiple of 4 the backward takes the one-workgroup-per-key-block kernels instead.
    split 2: the same shape on the 8-wave 256-key kernels (head_dim 32: the one-barrier fp16 backward, h16 4 / 0 its 4-wave and two-barrier
    forms); dh8 0: head_dim 48 on the 4-wave backward."""
    from gaot_amd import _lib
    B, S, H, Hkv = 4, 1024, 8, 8
    (q, k, v, go), ref64, ref32 = _case(B, S, H, Hkv, D)
    with _switches(**BIG_MODES[mode]):
        if mode == "keysplit2":
            assert _lib.load().gaot_attention_fwd_workspace(B, S, H, D) == 2 * (B * S * H * D + B * H * S)
        res = _call(layout, q, k, v, go, pieces=4)
    _check(f"{mode} {layout} D={D}", res, ref64, ref32, word_expected=True)


# ------------------------------------------------------------------------------------------------------------------
# B. grouped kv heads: one dK / dV block per query head
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,p_drop", [(32, 0.0), (64, 0.0), (128, 0.0), (192, 0.0), (64, 0.25), (192, 0.25)])
@pytest.mark.parametrize("Hkv", [2, 1])
def test_grouped_kv_heads(Hkv, D, p_drop):
    from gaot_amd import ops
    B, S, H = 1, 70, 8
    seed = 99 + D
    (q, k, v, go), ref64, ref32 = _case(B, S, H, Hkv, D, p_drop=p_drop, drop_seed=seed)
    for pieces in ((3,) if p_drop > 0.0 else (3, 4)):
        res = _call("separate-dense", q, k, v, go, pieces=pieces, p_drop=p_drop, drop_seed=seed)
        _check(f"group {H}/{Hkv} D={D} p={p_drop} pieces={pieces}", res, ref64, ref32, word_expected=pieces == 4)
    # through ops.attention: the gradient reduced over the group
    if p_drop > 0.0:
        ops.seed_dropout(4321, dev())
    via = _ops_attention(q, k, v, go, p_drop)
    if p_drop > 0.0:
        fac = _dropout_factor(int(ops._LAST_DROPOUT_SEED[0].cpu().item()), B, H, S, p_drop)
        ref64 = _closed_form(q, k, v, go, torch.float64, fac)
    errs = dict(o=_rel(via["o"], ref64["o"]), dq=_rel(via["dq"], ref64["dq"]),
                dk=_rel(via["dk"], _group_sum(ref64["dk"], Hkv)), dv=_rel(via["dv"], _group_sum(ref64["dv"], Hkv)))
    print(f"[group {H}/{Hkv} D={D} p={p_drop} ops] " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs["o"] < BAR_OUT and max(errs["dq"], errs["dk"], errs["dv"]) < BAR_GRAD, errs


# ------------------------------------------------------------------------------------------------------------------
# C. tile edges and the XCD branch, through ops.attention
# ------------------------------------------------------------------------------------------------------------------
def _ops_against_float64(tag, B, S, H, Hkv, D):
    (q, k, v, go), ref64, _ = _case(B, S, H, Hkv, D)
    via = _ops_attention(q, k, v, go)
    for t in via.values():
        assert bool(torch.isfinite(t).all()), tag
    refs = dict(o=ref64["o"], dq=ref64["dq"], dk=_group_sum(ref64["dk"], Hkv), dv=_group_sum(ref64["dv"], Hkv))
    if S == 1:
        # softmax == 1: out is v; dS = P (dP - delta) with dP = delta = <dO, v> is zero up to the rounding of two fp32 dot products of
        # length D, each within sqrt(D) * 2^-24 * sum |dO_d v_d| of the exact value (the statistical bound; the worst case is D * 2^-24),
        # so |dq| <= 2 sqrt(D) 2^-24 sum |dO v| * max |k| / sqrt(D), |dk| the same with max |q|
        r = H // Hkv
        vx = v.repeat_interleave(r, dim=2)
        dot = float((go.double() * vx.double()).abs().sum(-1).max())
        bar_q = 2 * 2.0 ** -24 * dot * float(k.abs().max())
        bar_k = 2 * 2.0 ** -24 * dot * float(q.abs().max()) * r
        off = (via["o"] - vx).abs()
        ulps = float((off / (2.0 ** (torch.floor(torch.log2(vx.abs().clamp_min(1e-30))) - 23))).max())
        print(f"[{tag}] |out - v| {float(off.max()):.2e} ({ulps:.1f} ulp)  |dq| {float(via['dq'].abs().max()):.2e} (bar {bar_q:.2e})  "
              f"|dk| {float(via['dk'].abs().max()):.2e} (bar {bar_k:.2e})")
        assert float(via["dq"].abs().max()) <= bar_q and float(via["dk"].abs().max()) <= bar_k, tag
        assert _rel(via["dv"], refs["dv"]) < BAR_GRAD, tag
        assert torch.equal(via["o"], vx), (tag, float(off.max()), ulps)
        return
    errs = {n: _rel(via[n], refs[n]) for n in refs}
    print(f"[{tag}] " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert errs["o"] < BAR_OUT and max(errs["dq"], errs["dk"], errs["dv"]) < BAR_GRAD, (tag, errs)


EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("S", EDGES)
def test_tile_edges(S, D):
    _ops_against_float64(f"edge S={S} D={D}", 1, S, 2, 1, D)


@pytest.mark.parametrize("split", [2, 0])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("S", EDGES)
def test_tile_edges_forced_kernels(S, D, split):
    with _switches(split=split):
        _ops_against_float64(f"edge S={S} D={D} split={split}", 1, S, 2, 1, D)


@pytest.mark.parametrize("S", [64, 130, 161])
@pytest.mark.parametrize("D", [160, 256])
@pytest.mark.parametrize("B,H,Hkv", [(1, 8, 8), (2, 8, 8), (3, 8, 8), (1, 8, 2), (2, 8, 2), (3, 8, 2), (3, 4, 2)])
def test_wide_kernels_on_the_xcd_branch(B, H, Hkv, D, S):
    """B*H = 8, 16, 24: xcd_group_decode deals the workgroups of one (batch, head) to one XCD; B*H = 12 is the other branch"""
    _ops_against_float64(f"xcd B*H={B * H} Hkv={Hkv} D={D} S={S}", B, S, H, Hkv, D)


# ------------------------------------------------------------------------------------------------------------------
# D. hard inputs per path
# ------------------------------------------------------------------------------------------------------------------
PATHS = {
    "D32": (32, {}, "fp16x2"), "D32-bf16x3": (32, {}, "bf16x3"), "D32-split0": (32, dict(split=0), "fp16x2"),
    "D48": (48, {}, "fp16x2"), "D64-split2": (64, dict(split=2), "fp16x2"), "D96": (96, {}, "fp16x2"),
    "D128": (128, {}, "fp16x2"), "D192": (192, {}, "fp16x2"), "D256": (256, {}, "fp16x2"),
}
INPUTS = ("peaked", "qk+1", "v+30", "qkx3", "vx30", "dout*1e-6")


@functools.lru_cache(maxsize=None)
def _hard_case(kind, S, H, Hkv, D):
    q, k, v, go = _randn_case(1, S, H, Hkv, D, 31 * D + Hkv)
    if kind == "peaked":
        q[0, 17, 0] *= 6.0
        k[0, S - 9, 0] = q[0, 17, 0] * 1.5
    elif kind == "qk+1":
        q, k = q + 1.0, k + 1.0
    elif kind == "v+30":
        v = v + 30.0
    elif kind == "qkx3":
        q, k = q * 3.0, k * 3.0
    elif kind == "vx30":
        v = v * 30.0
    elif kind == "dout*1e-6":
        go = go * 1e-6
    else:
        raise AssertionError(kind)
    r64, r32 = _closed_form(q, k, v, go, torch.float64), _closed_form(q, k, v, go, torch.float32)
    red = lambda r: dict(o=r["o"], dq=r["dq"], dk=_group_sum(r["dk"], Hkv), dv=_group_sum(r["dv"], Hkv))
    return (q, k, v, go), red(r64), red(r32)


@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_hard_inputs(path, kind, Hkv):
    D, sw, pieces = PATHS[path]
    (q, k, v, go), ref64, ref32 = _hard_case(kind, 160, 2, Hkv, D)
    with _switches(**sw), _f32_pieces(pieces):
        via = _ops_attention(q, k, v, go)
    failed = []
    for n in ("o", "dq", "dk", "dv"):
        assert bool(torch.isfinite(via[n]).all()), (path, kind, n)
        e, e32 = _rel(via[n], ref64[n]), _rel(ref32[n], ref64[n])
        bar = max(BAR_OUT if n == "o" else BAR_GRAD, 4 * e32)
        print(f"[hard {path} {kind} Hkv={Hkv}] {n}: kernel {e:.2e}  fp32 reference {e32:.2e}  ratio {e / e32:.2f}  bar {bar:.2e}")
        if not e <= bar:
            failed.append((n, e, e32, bar))
    assert not failed, (path, kind, Hkv, failed)
