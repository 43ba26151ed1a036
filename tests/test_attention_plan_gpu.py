"""-m gpu: one call per main-kernel family of csrc/attention_plan.h, forward and backward, each at the smallest shape that reaches the
family (found on the CPU from gaot_debug_attention_plan).  Every case goes through the harness of tests/test_attention_boundary_gpu.py
(guard bands, sentinels, float64 references) and asserts that the plan the launch EXECUTED (gaot_debug_last_attention_plan) is the dry
plan of the same call, that its family and template arguments are the ones the case names, and that o, lse, dq, dk, dv meet that
module's bars against float64 (BAR_OUT 3e-6, BAR_GRAD 1e-5).  Those bars are for fp32-level products, so every case asks for `pieces` 3 or
4; the two-rounded-piece instantiations (`pieces` 2: 16 significant bits per operand, e.g. attn_bwd_split8_dh_kernel<false, 1>) are
covered by the CPU table only."""
import ctypes as C

import pytest
import torch

from tests.test_attention_boundary_gpu import BAR_GRAD, _call, _case, _check, _rel, _switches

pytestmark = pytest.mark.gpu

SMALL, H16, HALF, FULL = (1, 129, 2, 2), (1, 513, 2, 2), (4, 512, 16, 16), (4, 1024, 16, 16)      # B, S, H, Hkv
# HALF: 128 workgroups of 256 keys / queries with two spare dQ slabs (key-split forward, query-split backward); FULL: 256 of them;
# H16: B H S >= 1 024, the floor of the attn_bwd_h16 kernels
# name: (shape, head_dim, pieces, switches, p_drop, forward family + arguments, backward family + arguments)
CASES = {
    "one-key": ((1, 1, 2, 2), 32, 3, {}, 0.0, ("OneKey", {}), ("BwdSplit4", {})),
    "fp32-31": (SMALL, 31, 3, {}, 0.0, ("Fp32", dict(dh=32, drop=0)), ("Fp32", dict(dh=32, drop=0, lds_bytes=59136))),
    "fp32-63": (SMALL, 63, 3, {}, 0.0, ("Fp32", dict(dh=64)), ("Fp32", dict(dh=64, reduce=2))),
    "fp32-96": (SMALL, 96, 3, {}, 0.0, ("Fp32", dict(dh=128)), ("Fp32", dict(dh=128, delta=1))),
    "glds": (SMALL, 32, 3, dict(split=0), 0.0, ("Glds", {}), ("Fp32", dict(dh=32))),
    "split4-32": (SMALL, 32, 4, {}, 0.0, ("Split", dict(nw=4, dh=32, pp=2, op=2, f16=1, ks=1)), ("BwdSplit4", dict(absmax_tensors=2))),
    "split4-48": (SMALL, 48, 4, {}, 0.0, ("Split", dict(nw=4, dh=64, pp=2, op=2, f16=1, ks=1)), ("BwdSplitDh", dict(dh=64, pp=2, op=2, f16=1))),
    "wide": (SMALL, 192, 3, {}, 0.0, ("Wide", dict(drop=0)), ("Wide", dict(drop=0, reduce=0))),
    "split8-32-f16": (SMALL, 32, 4, dict(split=2), 0.0, ("Split", dict(nw=8, dh=32, f16=1)), ("BwdSplit8", dict(pp=2, op=2, tr=1, f16=1, qs=1, delta=0))),
    "split8-32-bf16x3": (SMALL, 32, 3, dict(split=2), 0.0, ("Split", dict(nw=8, dh=32, pp=3, op=3, f16=0)), ("BwdSplit8", dict(pp=3, op=3, tr=0, f16=0, qs=1))),
    "split8-48-f16": (SMALL, 48, 4, dict(split=2), 0.0, ("Split", dict(nw=8, dh=64, pp=2, op=2, f16=1)), ("BwdSplitDh", dict(dh=64, f16=1))),
    "pipe": ((1, 128, 2, 2), 32, 3, dict(split=2, pipe=1), 0.0, ("Pipe", {}), ("BwdSplit8", dict(pp=3, op=3))),
    "h16-0x18": (H16, 32, 4, dict(split=2), 0.0, ("Split", dict(nw=8, dh=32, f16=1)), ("BwdH16", dict(nw=8, qs=1, var=1, delta=0, absmax_tensors=0))),
    "h16-4": (H16, 32, 4, dict(split=2, h16=4), 0.0, ("Split", dict(nw=8, dh=32, f16=1)), ("BwdH16", dict(nw=4, qs=1, var=0, n_kblocks=5))),
    "h16-0": (H16, 32, 4, dict(split=2, h16=0), 0.0, ("Split", dict(nw=8, dh=32, f16=1)), ("BwdSplit8", dict(pp=2, op=2, tr=1, f16=1, qs=1))),
    "keysplit-qsplit-48": (HALF, 48, 4, {}, 0.0, ("Split", dict(nw=8, dh=64, f16=1, ks=2, grid=256)), ("BwdSplit8Dh", dict(f16=1, qs=2, grid=256, n_kblocks=2))),
    "keysplit-qsplit-32": (HALF, 32, 4, dict(keysplit=2), 0.0, ("Split", dict(nw=8, dh=32, f16=1, ks=2, grid=256)), ("BwdSplit8", dict(f16=1, qs=2, grid=256, delta=0))),
    "split8-dh-full": (FULL, 48, 4, {}, 0.0, ("Split", dict(nw=8, dh=64, f16=1, ks=1, grid=256)), ("BwdSplit8Dh", dict(f16=1, qs=1, grid=256))),
    "dropout-fp32": (SMALL, 32, 3, {}, 0.25, ("Fp32", dict(dh=32, drop=1)), ("Fp32", dict(dh=32, drop=1, delta=2, reduce=2))),
    "dropout-wide": (SMALL, 192, 3, {}, 0.25, ("Wide", dict(drop=1)), ("Wide", dict(drop=1, delta=2))),
}


def _facts(lib, B, S, H, Hkv, D, pieces, dropout):
    """what the entry points read off the `separate-dense` layout of the harness: every base 16-byte aligned, every pitch its used columns"""
    from gaot_amd._lib import ATTENTION_FACTS
    on = dict.fromkeys(ATTENTION_FACTS, True)
    on["qkv_absmax"] = on["dout_absmax"] = on["dqkv_absmax"] = pieces == 4 and not dropout
    on["vec"] = (H * D) % 4 == 0 and (Hkv * D) % 4 == 0
    on["ldo4"] = on["lddq4"] = on["lddk4"] = on["lddv4"] = (H * D) % 4 == 0
    on["workspace"] = not dropout and lib.gaot_attention_fwd_workspace(B, S, H, D) > 0
    on["dq_part_aligned"] = (B * H * S) % 4 == 0
    return sum(1 << i for i, n in enumerate(ATTENTION_FACTS) if on[n])


@pytest.mark.parametrize("name", list(CASES))
def test_the_executed_plan_is_the_dry_plan_and_names_the_family(name):
    from gaot_amd import _lib
    from gaot_amd._lib import ATTENTION_FAMILIES, ATTENTION_PLAN_COLUMNS as PLAN, AttentionQuery
    lib = _lib.load()
    (B, S, H, Hkv), D, pieces, switches, p_drop, *expected = CASES[name]
    seed = 0x2468ace + D
    (q, k, v, go), ref64, ref32 = _case(B, S, H, Hkv, D, p_drop=p_drop, drop_seed=seed if p_drop else 0)
    with _switches(**switches):
        dry = []
        for direction in (0, 1):
            out = (C.c_int64 * len(PLAN))()
            call = AttentionQuery(B, S, H, Hkv, D, pieces, direction, int(p_drop > 0), _facts(lib, B, S, H, Hkv, D, pieces, p_drop > 0))
            _lib.check(lib.gaot_debug_attention_plan(C.byref(call), out), "gaot_debug_attention_plan")
            dry.append(dict(zip(PLAN, out)))
        res = _call("separate-dense", q, k, v, go, pieces=pieces, p_drop=p_drop, drop_seed=seed if p_drop else 0)
        for direction, (family, args) in enumerate(expected):
            out = (C.c_int64 * len(PLAN))()
            _lib.check(lib.gaot_debug_last_attention_plan(direction, out), "gaot_debug_last_attention_plan")
            ran = dict(zip(PLAN, out))
            assert ran == dry[direction], (name, direction)
            assert ATTENTION_FAMILIES[ran["family"]] == family, (name, direction, ran)
            assert {k_: ran[k_] for k_ in args} == args, (name, direction, ran)
    if S == 1:
        # softmax == 1 (the bars of test_attention_boundary_gpu._ops_against_float64): out is v bit for bit; dq and dk are zero up to the
        # rounding of the two fp32 dot products <dO, v> behind dP and delta
        vx = v.repeat_interleave(H // Hkv, dim=2)
        dot = float((go.double() * vx.double()).abs().sum(-1).max())
        assert torch.equal(res["o"], vx), name
        assert float(res["dq"].abs().max()) <= 2 * 2.0 ** -24 * dot * float(k.abs().max()), name
        assert float(res["dk"].abs().max()) <= 2 * 2.0 ** -24 * dot * float(q.abs().max()), name
        assert _rel(res["dv"], ref64["dv"]) < BAR_GRAD, name
        assert float((res["lse"].double() - ref64["lse"]).abs().max()) <= 4 * float((ref32["lse"].double() - ref64["lse"]).abs().max()) + 1e-6, name
        return
    _check(f"plan {name}", res, ref64, ref32, word_expected=pieces == 4 and not p_drop)
