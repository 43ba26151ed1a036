"""CPU side of sequential training from a PairStore (gaot_amd/sequential.py, csrc/seq_pairs.hip): the pair order and the per-pair tables
equal the reference's DynamicPairDataset's (tests/golden/seq_pairs.npz), the CPU store's batch equals EVERY recorded item bit for bit, the
constructor refuses what it cannot serve, the epoch's index lists cover the dataset once over the ranks, and the new entry points are
exported, declared and bound with matching arity inside ABI 10."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _seq_pairs as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = F.load_fixture()


def test_fixture_holds_the_cases_the_kernel_can_go_wrong_on():
    assert sorted(CASES) == ["n1_no_time_norm", "n257_truncated", "n67_output", "n67_residual", "n67_time_der"]
    c = CASES["n67_time_der"]
    assert tuple(c["u"].shape) == (3, 7, 67, 3) and tuple(c["c"].shape) == (3, 7, 67, 1) and tuple(c["x"].shape) == (18, 67, 6)
    assert (67 * 3) % 2 == 1 and c["x"].shape[-1] - 1 == 5          # N U and the conditioned-norm row width are odd
    assert sum(CASES[n]["x"].shape[0] for n in CASES if n.startswith("n67_")) == 54
    dt = c["t"][1:] - c["t"][:-1]
    assert float(dt.min()) > 0 and float(dt.max() - dt.min()) > 1e-3          # non-uniform time steps
    assert tuple(CASES["n1_no_time_norm"]["u"].shape) == (2, 5, 1, 1) and CASES["n1_no_time_norm"]["c"] is None
    t = CASES["n257_truncated"]
    assert tuple(t["u"].shape) == (2, 9, 257, 4) and int(t["t_out"].max()) == 4 and t["x"].shape[0] == 2 * 10          # T truncated to 5 steps


@pytest.mark.parametrize("name", sorted(CASES))
def test_time_pairs_and_tables_equal_the_reference(name):
    from gaot_amd.sequential import time_pairs
    c = CASES[name]
    store = F.make_store(c)
    nt = min(c["u"].shape[1] - 1, c["kw"]["max_time_diff"])
    t_in, t_out = time_pairs(nt, c["kw"]["time_step"])
    assert np.array_equal(t_in, c["t_in"]) and np.array_equal(t_out, c["t_out"])
    assert np.array_equal(store.t_in, c["t_in"]) and np.array_equal(store.t_out, c["t_out"])
    assert store.n_pairs == len(c["t_in"]) and len(store) == c["u"].shape[0] * store.n_pairs == c["x"].shape[0]
    assert torch.equal(store.start_times_norm, c["start_norm"]) and torch.equal(store.time_diffs_norm, c["diff_norm"])
    assert torch.equal(store.time_diffs, c["time_diffs"])
    assert store.start_times_norm.dtype == torch.float32
    if not c["kw"]["use_time_norm"]:
        assert torch.equal(store.start_times_norm, c["t"][c["t_in"]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_store_batch_equals_every_recorded_item(name):
    c = CASES[name]
    store = F.make_store(c)
    L = len(store)
    x, y = store.batch(list(range(L)))
    assert x.dtype == torch.float32 and torch.equal(x, c["x"]) and torch.equal(y, c["y"])
    order = list(range(L - 1, -1, -1)) + [0, 0, L - 1]          # descending, repeats
    x, y = store.batch(torch.tensor(order))
    assert torch.equal(x, c["x"][order]) and torch.equal(y, c["y"][order])
    xc, yc, cond = store.batch(order, conditional_norm=True)
    assert torch.equal(xc, c["x"][order][..., :-1]) and torch.equal(yc, c["y"][order]) and torch.equal(cond, c["x"][order][:, 0, -2:-1])
    with pytest.raises(IndexError):
        store.batch([L])
    x0, yseq = store.test_batch(list(range(c["u"].shape[0])), c["test_time_indices"])
    assert torch.equal(x0, c["test_x0"]) and torch.equal(yseq, c["test_yseq"])
    assert store.input_width() == c["x"].shape[-1] and store.input_width(True) == c["x"].shape[-1] - 1


def test_constructor_errors():
    from gaot_amd.sequential import PairStore
    c = CASES["n67_residual"]
    u, cc, t, stats = c["u"], c["c"], c["t"], c["stats"]
    with pytest.raises(ValueError, match="stats"):
        PairStore(u, cc, t, None)
    for mode, key in (("residual", "res"), ("time_der", "der")):
        with pytest.raises(ValueError, match=key):
            PairStore(u, cc, t, {k: v for k, v in stats.items() if k != key}, stepper_mode=mode)
    PairStore(u, cc, t, {k: v for k, v in stats.items() if k not in ("res", "der")}, stepper_mode="output")          # not needed: accepted
    with pytest.raises(ValueError, match="start_time"):
        PairStore(u, cc, t, {k: v for k, v in stats.items() if k != "start_time"})
    PairStore(u, cc, t, {k: v for k, v in stats.items() if k != "start_time"}, use_time_norm=False)
    with pytest.raises(ValueError, match="fp32"):
        PairStore(u.double(), cc, t, stats)
    with pytest.raises(ValueError, match="fp32"):
        PairStore(u, cc.half(), t, stats)
    with pytest.raises(ValueError, match="fp32"):
        PairStore(u, cc, t.double(), stats)
    with pytest.raises(ValueError, match="stepper_mode"):
        PairStore(u, cc, t, stats, stepper_mode="euler")
    with pytest.raises(ValueError):
        PairStore(u[:, :, :, 0], cc, t, stats)
    with pytest.raises(ValueError, match="no time pair"):
        PairStore(u[:, :2], cc[:, :2], t[:2], stats, time_step=2)
    with pytest.raises(RuntimeError, match="device tensors only"):
        s = F.make_store(c)
        s.compose(torch.zeros(1, dtype=torch.int32), torch.zeros(1, 67, 6), torch.zeros(1, 67, 3))


@pytest.mark.parametrize("world", [1, 2, 3])
def test_epoch_indices_cover_the_dataset_once_over_the_ranks(world):
    store = F.make_store(CASES["n257_truncated"])          # 20 items: 3 ranks need one item of padding
    L = len(store)
    per_rank = [store.epoch_indices(4, rank=r, world=world, seed=7) for r in range(world)]
    assert all(p.dtype == torch.int32 and p.device == store.device and p.numel() == -(-L // world) for p in per_rank)
    every = torch.stack(per_rank, dim=1).reshape(-1).tolist()          # rank-strided: the permutation itself, then the padding
    assert sorted(every[:L]) == list(range(L))
    assert every[L:] == every[:len(every) - L]          # shard_indices pads by repeating the head of the permutation
    # reproducible per (seed, epoch), different across epochs and seeds; unshuffled = the identity
    again = [store.epoch_indices(4, rank=r, world=world, seed=7) for r in range(world)]
    assert all(torch.equal(a, b) for a, b in zip(per_rank, again))
    assert not torch.equal(store.epoch_indices(5, 0, world, seed=7), per_rank[0])
    assert not torch.equal(store.epoch_indices(4, 0, world, seed=8), per_rank[0])
    assert store.epoch_indices(0, 0, 1, shuffle=False).tolist() == list(range(L))


def test_cpu_trainstep_runs_pair_batches_through_bind_pairs():
    """the gloo-side plumbing: a CPU model on a CPU store takes step_pairs, whole batches only"""
    from gaot_amd.trainer import TrainStep
    c = CASES["n67_output"]
    store = F.make_store(c)

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(6, 3)

        def forward(self, pndata):
            return self.lin(pndata)

    torch.manual_seed(0)
    m = Tiny()
    ts = TrainStep(m, lr=1e-2, use_graph=True)
    with pytest.raises(RuntimeError, match="bind_pairs"):
        ts.step_pairs([0, 1])
    ts.bind_pairs(store, 4)
    w0, b0 = m.lin.weight.detach().clone(), m.lin.bias.detach().clone()
    loss = ts.step_pairs([3, 17, 0, 3])
    want = torch.nn.functional.mse_loss(torch.nn.functional.linear(c["x"][[3, 17, 0, 3]], w0, b0), c["y"][[3, 17, 0, 3]])
    assert torch.equal(loss, want) and not torch.equal(m.lin.weight.detach(), w0)
    assert torch.equal(ts._x, c["x"][[3, 17, 0, 3]]) and torch.equal(ts._y, c["y"][[3, 17, 0, 3]])
    ts.step_pairs(torch.tensor([1, 2, 3, 4], dtype=torch.int32))
    assert torch.equal(ts._x, c["x"][1:5])
    with pytest.raises(ValueError, match="whole batches"):
        ts.step_pairs([1, 2, 3])
    ts.bind(c["x"][:2], c["y"][:2])          # back on caller-supplied batches
    with pytest.raises(RuntimeError, match="bind_pairs"):
        ts.step_pairs([0, 1])


def test_new_entries_exported_and_declared_with_matching_arity():
    from gaot_amd import build as B
    from gaot_amd import _lib
    assert "seq_pairs.hip" in B.ALL_SOURCES and B.ALL_SOURCES[:len(B.SOURCES)] == B.SOURCES
    B.build(verbose=False)
    lib = _lib.load()
    assert lib.gaot_abi_version() == 10                                        # additions only
    header = open(os.path.join(ROOT, "include", "gaot_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gaot_seq_pairs_compose", "gaot_seq_test_compose"):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gaot_hip.h"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
        assert "gaot_stream_t" in m.group(1).split(",")[-1] and "status_flag" in m.group(1).split(",")[-2]
    # the argument checks come before the launch: a bad call is refused without a device
    rc = lib.gaot_seq_pairs_compose(None, None, 1, 2, 1, 1, 0, None, None, None, None, None, 1, None, None, None, None, None, None, 0, 2, None, 1,
                                    None, None, None, None, None)
    assert rc != 0 and b"seq_pairs_compose" in lib.gaot_last_error()
