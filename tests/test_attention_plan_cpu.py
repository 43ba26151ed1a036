"""The attention kernel-selection table, enumerated without a GPU (csrc/attention_plan.h through gaot_debug_attention_plan and the two
workspace queries).

tests/golden/attention_plans.json is the record of the dispatch as it stood BEFORE the selection became one function: the four entry
points of attention.hip, compiled for the host with every launch replaced by a recorder, run over a grid of sizes (B 1 .. 16, S 1 .. 4 096
around every tile edge, H 1 .. 64, grouped kv heads, head_dim 1 .. 256), `pieces`, both directions, dropout, every subset of the absmax
pointers and every alignment fact on and off, under 36 settings of the debug switches -- and thinned so that every distinct plan a
setting produces (sizes aside) appears under that setting at least once.  tests/golden/attention_products.json holds the attention calls
of the bench configurations C2 .. C5 as ops.attention makes them in a training step, with the plan the same recorders saw.  A rule that
moves a call to another kernel, grid, slab count or workspace offset fails here, with the call in the message."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SWITCHES = ["split", "keysplit", "dh8", "h16", "p_pieces", "operand_pieces", "tr", "qsplit", "pipe"]
DEFAULTS = [1, 1, 1, 0x18, -1, -1, 1, 1, 0]
CALL = ["B", "S", "H", "Hkv", "head_dim", "pieces", "direction", "dropout", "facts"]
N_SETTINGS, ROWS_FLOOR = 36, 6700          # the floor: the thinned file holds 6 781 (setting, row) pairs over 635 distinct rows


@pytest.fixture(scope="module")
def lib():
    from gaot_amd.build import build
    from gaot_amd import _lib
    build(verbose=False)
    return _lib.load()


class switches:
    """the nine selection switches set together; the previous values come back in __exit__ whatever happens inside"""

    def __init__(self, lib, values):
        self.lib, self.values = lib, values

    def __enter__(self):
        self.old = []
        try:
            for name, v in zip(SWITCHES, self.values):
                self.old.append(getattr(self.lib, "gaot_debug_set_attention_" + name)(v))
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for name, v in zip(SWITCHES, self.old):
            getattr(self.lib, "gaot_debug_set_attention_" + name)(v)


def _plan(lib, call, rc_only=False):
    from gaot_amd._lib import ATTENTION_PLAN_COLUMNS, AttentionQuery
    out = (C.c_int64 * len(ATTENTION_PLAN_COLUMNS))()
    rc = lib.gaot_debug_attention_plan(C.byref(AttentionQuery(*call)), out)
    if rc_only:
        return rc
    assert rc == 0, (rc, lib.gaot_last_error())
    return list(out)


def _last(lib, direction):
    from gaot_amd._lib import ATTENTION_PLAN_COLUMNS
    out = (C.c_int64 * len(ATTENTION_PLAN_COLUMNS))()
    assert lib.gaot_debug_last_attention_plan(direction, out) == 0
    return list(out)


def _say(call):
    from gaot_amd._lib import ATTENTION_FACTS
    d = dict(zip(CALL, call))
    d["facts"] = "|".join(n for i, n in enumerate(ATTENTION_FACTS) if call[8] >> i & 1) or "none"
    return d


def test_every_plan_of_the_grid_under_every_switch_setting(lib):
    from gaot_amd._lib import ATTENTION_PLAN_COLUMNS as PLAN
    t = json.load(open(os.path.join(GOLDEN, "attention_plans.json")))
    assert t["columns"] == CALL + ["fwd_workspace", "bwd_workspace"] + PLAN and t["switches"] == SWITCHES
    assert len(t["settings"]) == N_SETTINGS and t["settings"][0]["set"] == DEFAULTS
    checked = 0
    for setting in t["settings"]:
        with switches(lib, setting["set"]):
            for i in setting["rows"]:
                row = t["rows"][i]
                call, (wf, wb), want = row[:9], row[9:11], row[11:]
                what = f"{_say(call)} under {dict(zip(SWITCHES, setting['set']))}"
                got = _plan(lib, call)
                assert got == want, f"{what}: {dict(zip(PLAN, got))}, recorded {dict(zip(PLAN, want))}"
                B, S, H, _, D = call[:5]
                assert lib.gaot_attention_fwd_workspace(B, S, H, D) == wf and lib.gaot_attention_bwd_workspace(B, S, H, D) == wb, what
                checked += 1
    assert checked >= ROWS_FLOOR
    assert [getattr(lib, "gaot_debug_set_attention_" + s)(v) for s, v in zip(SWITCHES, DEFAULTS)] == DEFAULTS          # every switch is back where it was


def test_the_model_calls_keep_their_kernels(lib):
    from gaot_amd._lib import ATTENTION_FAMILIES, ATTENTION_PLAN_COLUMNS as PLAN
    t = json.load(open(os.path.join(GOLDEN, "attention_products.json")))
    assert sorted(t["products"]) == ["C2", "C3", "C4", "C5"]
    with switches(lib, DEFAULTS):
        for cfg, rows in t["products"].items():
            assert len(rows) >= 2
            for call, want in rows:
                got = _plan(lib, call)
                assert got == want, f"{cfg} {_say(call)}: {dict(zip(PLAN, got))}, recorded {dict(zip(PLAN, want))}"
        # the flagship's kernels as the committed trace names them (profiles/r7b_step_sequence.txt): attn_fwd_split_kernel<8, 32, 2, 2, true, 1>,
        # attn_bwd_h16_kernel<8, 1, 1>, attn_dq_reduce_vec_kernel<8>
        fwd, bwd = (dict(zip(PLAN, _plan(lib, call))) for call, _ in t["products"]["C2"][:2])
        assert ATTENTION_FAMILIES[fwd["family"]] == "Split" and [fwd[k] for k in ("nw", "dh", "pp", "op", "f16", "ks")] == [8, 32, 2, 2, 1, 1]
        assert ATTENTION_FAMILIES[bwd["family"]] == "BwdH16" and [bwd[k] for k in ("nw", "qs", "var")] == [8, 1, 1]
        assert (bwd["delta"], bwd["reduce"], bwd["reduce_dp4"], bwd["absmax_tensors"]) == (0, 1, 8, 0)


def test_bad_sizes_have_no_plan_and_the_last_plan_stays(lib):
    t = json.load(open(os.path.join(GOLDEN, "attention_plans.json")))
    assert len(t["bad"]) >= 40
    before = [_last(lib, 0), _last(lib, 1)]
    for *call, rc, message in t["bad"]:
        assert _plan(lib, call + [0x7fff], rc_only=True) == rc != 0, call
        assert lib.gaot_last_error().decode() == message, call
    assert [_last(lib, 0), _last(lib, 1)] == before
    assert lib.gaot_debug_attention_plan(None, (C.c_int64 * 31)()) != 0
    good = [2, 64, 4, 2, 32, 3, 0, 0, 0x7fff]
    assert _plan(lib, good)[2] == 4          # (the same call with good sizes has one: the split family)
    assert _plan(lib, good[:6] + [2, 0, 0x7fff], rc_only=True) != 0 and _plan(lib, good[:7] + [2, 0x7fff], rc_only=True) != 0


def test_the_setters_return_what_they_returned(lib):
    """recorded before the switches moved into one struct: p_pieces normalises (3 -> 33, 2 -> 22, anything but 22 / 23 / 32 / 33 -> -1), so
    do operand_pieces (2, 3, else -1), tr and qsplit (0 / 1); the others echo their argument"""
    t = json.load(open(os.path.join(GOLDEN, "attention_plans.json")))
    assert sorted(t["echo"]) == sorted(SWITCHES)
    with switches(lib, DEFAULTS):
        for name, default in zip(SWITCHES, DEFAULTS):
            fn = getattr(lib, "gaot_debug_set_attention_" + name)
            assert len(t["echo"][name]) >= 18
            for arg, back in t["echo"][name]:
                fn(arg)
                assert fn(default) == back, (name, arg)
        assert dict(t["echo"]["p_pieces"])[3] == 33 and dict(t["echo"]["p_pieces"])[2] == 22 and dict(t["echo"]["p_pieces"])[77] == -1
        assert dict(t["echo"]["tr"])[77] == 1 and dict(t["echo"]["qsplit"])[-1] == 1 and dict(t["echo"]["split"])[77] == 77
    assert [getattr(lib, "gaot_debug_set_attention_" + s)(v) for s, v in zip(SWITCHES, DEFAULTS)] == DEFAULTS
