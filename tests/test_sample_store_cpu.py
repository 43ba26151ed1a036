"""No GPU needed: the host side of index-driven static training -- the capacity rule of the one union that serves a whole split
(graphs.batch_edge_capacity), the epoch partitioning and the CPU form of static.SampleStore, the refusals, and the two new entry points'
export and declaration.  The kernels themselves: tests/test_sample_store_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacity_is_the_bucket_of_the_b_largest_counts():
    from gaot_amd.graphs import batch_edge_capacity
    from gaot_amd.plan import edge_bucket
    counts = [5000, 120000, 7000, 90000, 30000, 64000]
    assert batch_edge_capacity(counts, 1) == edge_bucket(120000)
    assert batch_edge_capacity(counts, 3) == edge_bucket(120000 + 90000 + 64000)
    assert batch_edge_capacity(torch.tensor(counts), 6) == batch_edge_capacity(np.array(counts), 6) == edge_bucket(sum(counts))
    # every batch of B distinct samples fits, and the largest one is not padded by more than a bucket step (5 significant bits)
    rng = np.random.default_rng(0)
    for _ in range(50):
        pick = rng.choice(len(counts), size=3, replace=False)
        assert sum(counts[i] for i in pick) <= batch_edge_capacity(counts, 3)
    top = 120000 + 90000 + 64000
    assert top <= batch_edge_capacity(counts, 3) < top * (1 + 1 / 16)
    # tiny graphs: the bucket's floor
    assert batch_edge_capacity([3, 0, 9], 2) == edge_bucket(12) == 1024
    # B > S: no batch of distinct samples exists; an epoch's padded order repeats the list, so the counts are cycled, largest first
    assert batch_edge_capacity(counts, 8) == edge_bucket(sum(counts) + 120000 + 90000)
    assert batch_edge_capacity([7000], 4) == edge_bucket(28000)
    with pytest.raises(ValueError, match="at least one"):
        batch_edge_capacity(counts, 0)
    with pytest.raises(ValueError, match="at least one"):
        batch_edge_capacity([], 2)


def test_capacity_from_2_to_the_31_on_is_refused():
    from gaot_amd.graphs import batch_edge_capacity
    big = (1 << 30) - 1
    assert batch_edge_capacity([big, 5], 1) < (1 << 31)
    with pytest.raises(ValueError, match="2\\^31"):
        batch_edge_capacity([big, big, big], 2)          # 2^31 - 2 edges: its bucket is 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        batch_edge_capacity([1 << 31], 1)
    with pytest.raises(ValueError, match="2\\^31"):
        batch_edge_capacity([1 << 20] * 4, 4096)          # B > S, summed in 64 bits


def _fx_store(S=7, N=11, Cc=3, U=2, seed=0):
    from gaot_amd.static import SampleStore
    g = torch.Generator().manual_seed(seed)
    c, u, coord = torch.randn(S, N, Cc, generator=g), torch.randn(S, N, U, generator=g), torch.rand(N, 2, generator=g)
    return SampleStore(c, u, coord=coord), c, u, coord


def test_epoch_indices_partition_the_samples_like_shard_indices():
    from gaot_amd.trainer import shard_indices
    store, _, _, _ = _fx_store()
    S, world = len(store), 3
    assert S == 7
    per_rank = [store.epoch_indices(4, rank=r, world=world, seed=7) for r in range(world)]
    for r, p in enumerate(per_rank):
        assert p.dtype == torch.int32 and p.device == store.device and p.tolist() == shard_indices(S, r, world, 4, True, 7)
    every = torch.stack(per_rank, dim=1).reshape(-1).tolist()          # rank-strided: the permutation itself, then the padding
    assert sorted(every[:S]) == list(range(S)) and every[S:] == every[:len(every) - S]
    assert not torch.equal(store.epoch_indices(5, 0, world, seed=7), per_rank[0])
    assert store.epoch_indices(0, 0, 1, shuffle=False).tolist() == list(range(S))


def test_cpu_store_compose_is_plain_indexing_and_feeds_a_cpu_trainstep():
    from gaot_amd.trainer import TrainStep
    store, c, u, coord = _fx_store()
    assert not store.vx and store.device.type == "cpu" and store.status() == 0
    for lst in ([6], [2, 0, 2, 5, 1]):
        idx = torch.tensor(lst, dtype=torch.int32)
        x, y = torch.full((len(lst), 11, 3), -7.0), torch.full((len(lst), 11, 2), -7.0)
        store.compose(idx, x, y)
        assert torch.equal(x, c[lst]) and torch.equal(y, u[lst])
    with pytest.raises(IndexError):
        store.compose(torch.tensor([7], dtype=torch.int32), x[:1], y[:1])
    with pytest.raises(ValueError, match="contiguous"):
        store.compose(torch.tensor([1], dtype=torch.int64), x[:1], y[:1])
    with pytest.raises(ValueError, match="xcoord"):
        store.compose(torch.tensor([1], dtype=torch.int32), x[:1], y[:1], torch.zeros(1, 11, 2))

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(3, 2)

        def forward(self, pndata, xcoord):
            assert xcoord.shape == (11, 2)
            return self.lin(pndata)

    torch.manual_seed(0)
    m = Tiny()
    ts = TrainStep(m, lr=1e-2, use_graph=True)
    with pytest.raises(RuntimeError, match="bind_samples"):
        ts.step_samples([0, 1])
    ts.bind_samples(store, 4)
    w0, b0 = m.lin.weight.detach().clone(), m.lin.bias.detach().clone()
    loss = ts.step_samples([3, 6, 0, 3])
    want = torch.nn.functional.mse_loss(torch.nn.functional.linear(c[[3, 6, 0, 3]], w0, b0), u[[3, 6, 0, 3]])
    assert torch.equal(loss, want) and not torch.equal(m.lin.weight.detach(), w0)
    ts.step_samples(store.epoch_indices(0, shuffle=False)[1:5])
    assert torch.equal(ts._x, c[1:5]) and torch.equal(ts._y, u[1:5])
    with pytest.raises(ValueError, match="whole batches"):
        ts.step_samples([1, 2, 3])
    ts.bind(c[:2], u[:2])          # back on caller-supplied batches
    with pytest.raises(RuntimeError, match="bind_samples"):
        ts.step_samples([0, 1])


def test_refusals():
    from gaot_amd.graphs import GraphBuilder
    from gaot_amd.static import SampleStore
    g = torch.Generator().manual_seed(1)
    c, u, coord = torch.randn(4, 9, 3, generator=g), torch.randn(4, 9, 1, generator=g), torch.rand(9, 2, generator=g)
    with pytest.raises(ValueError, match="c_data is required"):
        SampleStore(None, u, coord=coord)
    with pytest.raises(ValueError, match="4 samples, u_data 3"):
        SampleStore(c, u[:3], coord=coord)
    with pytest.raises(ValueError, match="nodes per sample"):
        SampleStore(c, u[:, :8], coord=coord)
    with pytest.raises(ValueError, match="fp32"):
        SampleStore(c.double(), u, coord=coord)
    with pytest.raises(ValueError, match="exactly one"):
        SampleStore(c, u)
    with pytest.raises(ValueError, match="coord must be"):
        SampleStore(c, u, coord=coord[:8])
    # vx over a GraphStore built on the host: no arenas to index into, no fallback
    x = torch.rand(4, 9, 2, generator=g)
    lat = torch.stack(torch.meshgrid(torch.linspace(-1, 1, 4), torch.linspace(-1, 1, 4), indexing="ij"), -1).reshape(-1, 2)
    host = GraphBuilder().build_store(x, lat, 0.7, [1.0])
    with pytest.raises(RuntimeError, match="device tensors"):
        SampleStore(c, u, graphs=host)
    with pytest.raises(RuntimeError, match="host tensors"):
        host.part_table(0, "encoder")
    with pytest.raises(ValueError, match="side"):
        host.part_table(0, "both")
    assert host.batch_edge_capacity(2, 0) == 1024          # (the counts are the host's in either kind of store)


def test_new_entries_exported_and_declared_with_matching_arity():
    from gaot_amd import build as B
    from gaot_amd import _lib
    assert "sample_store.hip" in B.ALL_SOURCES and "sample_store.hip" not in B.SOURCES
    assert B.ALL_SOURCES[:len(B.SOURCES)] == B.SOURCES and len(B.SOURCES) == 16
    assert os.path.exists(os.path.join(B.CSRC, "sample_store.hip"))
    B.build(verbose=False)
    lib = _lib.load()
    assert lib.gaot_abi_version() == 10                                        # additions only
    header = open(os.path.join(ROOT, "include", "gaot_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gaot_union_compose_indexed", "gaot_sample_gather"):
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gaot_hip.h"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
    # the argument checks come before any launch: bad calls are refused without a device
    assert lib.gaot_sample_gather(None, None, None, 4, 8, 3, 1, 0, None, 2, None, None, None, None, None) != 0
    assert b"sample_gather" in lib.gaot_last_error()
    assert lib.gaot_union_compose_indexed(None, 4, None, 2, 8, 8, 2, 2, 64, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"union_compose_indexed" in lib.gaot_last_error()
