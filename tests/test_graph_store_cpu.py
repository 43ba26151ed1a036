"""CPU side of the dataset-level graph builder (gaot_amd/graphs.py, csrc/graph_store.hip): GraphBuilder on host tensors reproduces what
the reference's GraphBuilder (neighbor_search_method="grid") and rescale gave on the recorded point sets (tests/golden/graph_builder.npz,
written by tests/golden/make_graph_builder.py) -- row splits equal, every row equal as a sorted list (the reference's grid backend lists a
row cell by cell), x_scaled bit-equal --, the two methods keep the reference's signatures and errors, and the new entry points are
exported, declared and bound inside ABI 10."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "graph_builder.npz"))
    scales = [float(v) for v in z["scales"]]
    out = {}
    for name in (str(n) for n in z["cases"]):
        x = torch.from_numpy(z[f"{name}/x"])
        S = x.shape[0]
        side = lambda sd: [[(torch.from_numpy(z[f"{name}/{sd}/{s}/{k}/index"]), torch.from_numpy(z[f"{name}/{sd}/{s}/{k}/splits"]))
                            for k in range(len(scales))] for s in range(S)]
        out[name] = dict(x=x, latent=torch.from_numpy(z[f"{name}/latent"]), radius=float(z[f"{name}/radius"]),
                         x_scaled=torch.from_numpy(z[f"{name}/x_scaled"]), enc=side("enc"), dec=side("dec"))
    return scales, out


SCALES, CASES = _fixture()


def _sorted_rows(idx, sp):
    return [sorted(idx[int(sp[i]):int(sp[i + 1])].tolist()) for i in range(sp.numel() - 1)]


def test_fixture_holds_the_recorded_cases():
    assert SCALES == [1.0, 1.5] and sorted(CASES) == ["d2", "d3"]
    assert tuple(CASES["d2"]["x"].shape) == (3, 200, 2) and tuple(CASES["d3"]["x"].shape) == (2, 1, 150, 3)
    assert float(CASES["d2"]["x"][1, :, 1].max() - CASES["d2"]["x"][1, :, 1].min()) == 0.0          # the zero-range branch of rescale
    assert bool((CASES["d2"]["x_scaled"][1, :, 1] == -1.0).all())
    edges = sum(int(i.numel()) for c in CASES.values() for row in c["enc"] for i, _ in row)
    assert 500 < edges < 6000
    # the reference's rows really are not sorted everywhere: comparing rows as sorted lists is needed
    raw_rows = lambda i, s: [i[int(s[j]):int(s[j + 1])].tolist() for j in range(s.numel() - 1)]
    assert any(_sorted_rows(i, s) != raw_rows(i, s) for row in CASES["d2"]["enc"] for i, s in row)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_builder_reproduces_the_reference(name):
    from gaot_amd.graphs import GraphBuilder
    c = CASES[name]
    b = GraphBuilder(neighbor_search_method="grid")
    store = b.build_store(c["x"], c["latent"], c["radius"], SCALES)
    S = c["x"].shape[0]
    assert store.x_scaled.dtype == torch.float32 and torch.equal(store.x_scaled, c["x_scaled"])
    assert tuple(store.edge_counts.shape) == (S, len(SCALES)) and store.edge_counts.dtype == torch.int64
    assert store.nbytes > store.x_scaled.numel() * 4
    enc, dec = b.build_graphs_for_split(c["x"], c["latent"], c["radius"], SCALES)
    for got, want in ((store.encoder, c["enc"]), (store.decoder, c["dec"]), (enc, c["enc"]), (dec, c["dec"])):
        assert len(got) == S and all(len(row) == len(SCALES) for row in got)
        for s in range(S):
            for k in range(len(SCALES)):
                idx, sp = got[s][k]["neighbors_index"], got[s][k]["neighbors_row_splits"]
                widx, wsp = want[s][k]
                assert idx.dtype == torch.int64 and sp.dtype == torch.int64
                assert torch.equal(sp, wsp), (name, s, k)
                rows = _sorted_rows(widx, wsp)
                assert [idx[int(sp[i]):int(sp[i + 1])].tolist() for i in range(sp.numel() - 1)] == rows, (name, s, k)          # ascending here
    for s in range(S):
        for k in range(len(SCALES)):
            assert int(store.edge_counts[s, k]) == store.encoder[s][k]["neighbors_index"].numel() == store.decoder[s][k]["neighbors_index"].numel()


def test_build_all_graphs_keeps_the_reference_structure():
    from gaot_amd.graphs import GraphBuilder
    c = CASES["d2"]
    b = GraphBuilder()
    splits = {"train": {"x": c["x"][:2]}, "val": {"x": c["x"][2:]}, "test": {"x": c["x"][1:]}}
    full = b.build_all_graphs(splits, c["latent"], c["radius"], SCALES)
    assert sorted(full) == ["test", "train", "val"]
    assert len(full["train"]["encoder"]) == 2 and len(full["val"]["decoder"]) == 1 and len(full["test"]["encoder"]) == 2
    assert torch.equal(full["val"]["encoder"][0][1]["neighbors_row_splits"], c["enc"][2][1][1])
    only = b.build_all_graphs(splits, c["latent"], c["radius"], SCALES, build_train=False)
    assert only["train"] is None and only["val"] is None and len(only["test"]["decoder"]) == 2
    assert torch.equal(only["test"]["decoder"][0][0]["neighbors_row_splits"], c["dec"][1][0][1])
    assert "train" not in b.build_all_graphs({"test": splits["test"]}, c["latent"], c["radius"], SCALES)


def test_bad_shape_and_capped_method_are_refused():
    from gaot_amd.graphs import GraphBuilder
    c = CASES["d2"]
    b = GraphBuilder()
    with pytest.raises(ValueError, match="Unexpected coordinate shape"):
        b.build_graphs_for_split(c["x"][0], c["latent"], c["radius"], SCALES)                      # [N, d]
    with pytest.raises(ValueError, match="Unexpected coordinate shape"):
        b.build_graphs_for_split(c["x"][:, None].repeat(1, 2, 1, 1), c["latent"], c["radius"], SCALES)          # [S, 2, N, d]
    with pytest.raises(NotImplementedError, match="NeighborSearch"):
        GraphBuilder(neighbor_search_method="torch_cluster")
    with pytest.raises(ValueError):
        GraphBuilder(neighbor_search_method="kdtree")
    for m in ("auto", "native", "grid", "chunked", "open3d"):
        GraphBuilder(neighbor_search_method=m)


def test_plan_from_arrays_is_a_classmethod_beside_the_composed_path():
    from gaot_amd.plan import GeometryPlan
    t = torch.zeros(1, dtype=torch.int32)
    p = GeometryPlan.from_arrays(3, 0, 2, t, torch.zeros(4, dtype=torch.int32), t, torch.zeros(3, dtype=torch.int32), t,
                                 torch.zeros(3, dtype=torch.int64), 5, 7)
    assert (p.Q, p.E, p.n_src, p.max_deg, p.max_t_deg) == (3, 0, 2, 0, 0) and p._src_id is None and not p.rows_skewed
    idx = torch.zeros(4, dtype=torch.int64)
    p = GeometryPlan.from_arrays(3, 4, 2, t, t, t, t, t, t, 60, 2, index_long=idx, src_index=idx)
    assert p._src_id == (id(idx), idx._version) and p.rows_skewed and not p.t_rows_skewed and p.index_long is idx


def test_new_entries_exported_and_declared_with_matching_arity():
    from gaot_amd import build as B
    from gaot_amd import _lib
    assert "graph_store.hip" in B.ALL_SOURCES and B.ALL_SOURCES[:len(B.SOURCES)] == B.SOURCES and len(B.SOURCES) == 16
    B.build(verbose=False)
    lib = _lib.load()
    assert lib.gaot_abi_version() == 10                                        # additions only
    header = open(os.path.join(ROOT, "include", "gaot_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("gaot_rescale_batch", "gaot_graph_store_scratch", "gaot_graph_store_count", "gaot_graph_store_fill"):
        assert hasattr(lib, name), name
        m = re.search(r"\bint(?:64_t)?\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gaot_hip.h"
        restype, argtypes = _lib.PROTOTYPES[name]
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(argtypes), name
    # the argument checks come before any launch: bad calls are refused without a device
    assert lib.gaot_rescale_batch(None, 1, 1, 2, None, None) != 0 and b"rescale_batch" in lib.gaot_last_error()
    assert lib.gaot_graph_store_scratch(4, 100, 49, 4, 0.1) == -1 and b"dim 2 or 3" in lib.gaot_last_error()
    assert lib.gaot_graph_store_scratch(1 << 20, 8192, 4096, 2, 0.1) == -1 and b"2^31" in lib.gaot_last_error()
    small, big = lib.gaot_graph_store_scratch(4, 100, 49, 2, 0.5), lib.gaot_graph_store_scratch(8, 100, 49, 2, 0.5)
    assert 0 < small < big and small % 8 == 0
    assert lib.gaot_graph_store_count(None, 4, 100, None, 49, 2, 0.5, None, None, None, None, None, None, None) != 0
    assert b"graph_store_count" in lib.gaot_last_error()
    assert lib.gaot_graph_store_fill(None, 4, 100, None, 49, 2, -1.0, None, 0, 0, 0, None, None, None, None, None, None, None, None, None, None,
                                     None, None, None) != 0
    assert b"radius" in lib.gaot_last_error()
