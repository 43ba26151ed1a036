"""GraphBuilder: the encoder / decoder radius graphs of a whole variable-coordinate (vx) dataset split.

The reference's GraphBuilder (src/datasets/graph_builder.py:13-144) loops over the samples in Python: rescale to [-1, 1], then
2 x len(scales) radius searches against the shared latent grid.  Here the same two methods, with the same signatures and the same
reference-style dicts, are served by a GraphStore:

  * device inputs: a FIXED number of launches for the whole split (csrc/graph_store.hip) -- one batched rescale, and per scale one
    count pass, one readback of the per-sample edge counts and maximum degrees (all scales in one transfer), and one fill pass.
    The lists of all samples live in a few arenas; every dict tensor is a view, and every dict carries a full GeometryPlan
    (plan.GeometryPlan.from_arrays) whose arrays are views too: training composes its unions from them from the first step on,
    without gaot_csr_prepare / gaot_csr_transpose and without a validation sync -- the lists are valid by construction;
  * host inputs: the per-sample loop over the rescale expression and NeighborSearch (CPU tests, dataset preparation on a host).
    There is no fallback from the device path to this one.

Rows are in ascending neighbour index.  The exact uncapped methods are served; 'torch_cluster' (capped at 32, strict, not
symmetric) is not a dataset-level build: use NeighborSearch(method='torch_cluster') per sample.
"""
from typing import List, Tuple

import numpy as np
import torch

from .model.layers.utils.neighbor_search import NeighborSearch

_EXACT = ("auto", "native", "grid", "chunked", "open3d")
# kernels per C entry point, COUNTED FROM THE CODE of csrc/graph_store.hip (not measured): count = zero, cell count / scan / fill, walk,
# two row scans; fill = walk, absolute starts, two launches per segment sort x two directions, link.  The C entry points only: per
# scale the build also issues two torch subtractions (the int64 row lengths) and one host-to-device copy (the arena offsets).
LAUNCHES_RESCALE, LAUNCHES_COUNT, LAUNCHES_FILL = 1, 7, 7


def _alloc(*shape, dtype, device) -> torch.Tensor:
    """every device allocation of a build, scratch included (one place, so a test can hand out pre-filled memory)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def rescale(x: torch.Tensor) -> torch.Tensor:
    """scaling.rescale(x, (-1, 1)) of the reference (src/utils/scaling.py:10-35) for one [N, d] sample, the same tensor expression"""
    lo = torch.min(x, dim=0, keepdim=True)[0]
    hi = torch.max(x, dim=0, keepdim=True)[0]
    rng = hi - lo
    rng = torch.where(rng == 0, torch.ones_like(rng), rng)
    return ((x - lo) / rng) * (1 - (-1)) + (-1)


def _samples(x_data: torch.Tensor) -> torch.Tensor:
    """[S, N, d] or [S, 1, N, d] -> [S, N, d]; anything else is the reference's ValueError (graph_builder.py:50-57)"""
    if x_data.dim() == 4 and x_data.shape[1] == 1:
        return x_data[:, 0]
    if x_data.dim() == 3:
        return x_data
    raise ValueError(f"Unexpected coordinate shape: {x_data.shape[1:]}")


class GraphStore:
    """The graphs of one split.  `encoder[s][k]` / `decoder[s][k]`: reference-style dicts (int64 neighbors_index, neighbors_row_splits)
    of sample s at scale k; `x_scaled` [S, N, d] fp32: the rescaled coordinates they were built from; `edge_counts`: host int64
    [S, len(scales)]; `nbytes`: what the store holds; `launches`: kernels the C entry points launched for the build, counted from their code
    (device stores; see LAUNCHES_*)."""

    def __init__(self, x_data: torch.Tensor, latent_queries: torch.Tensor, radii: List[float], method: str = "auto"):
        x = _samples(x_data)
        self.S, self.N, self.dim = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
        self.Q = int(latent_queries.shape[0])
        self.radii = [float(r) for r in radii]
        self.encoder: List[list] = [[] for _ in range(self.S)]
        self.decoder: List[list] = [[] for _ in range(self.S)]
        self._arenas: List[dict] = []
        self.launches = 0
        if x.is_cuda != latent_queries.is_cuda:
            raise ValueError("GraphStore: coordinates and latent queries must live on the same device")
        if x.is_cuda:
            self._build_device(x, latent_queries)
        else:
            self._build_host(x, latent_queries, method)

    # ---- host tensors: the reference's loop
    def _build_host(self, x, latent, method):
        search = NeighborSearch(method)
        x = x.float()
        latent = latent.float()
        self.x_scaled = torch.stack([rescale(x[s]) for s in range(self.S)]) if self.S else x.clone()
        counts = np.zeros((self.S, len(self.radii)), dtype=np.int64)
        for s in range(self.S):
            xs = self.x_scaled[s]
            for k, r in enumerate(self.radii):
                enc = search(xs, latent, r)
                dec = search(latent, xs, r)
                self.encoder[s].append(enc)
                self.decoder[s].append(dec)
                counts[s, k] = enc["neighbors_index"].numel()
        self.edge_counts = torch.from_numpy(counts)
        held = [self.x_scaled] + [t for rows in (self.encoder, self.decoder) for row in rows for d in row for t in d.values()]
        self.nbytes = sum(t.numel() * t.element_size() for t in held)

    # ---- device tensors: batched kernels
    def _build_device(self, x, latent):
        from . import _lib as L
        from . import plan as P
        from .ops import _p, _stream
        lib = L.load()
        S, N, Q, dim, K = self.S, self.N, self.Q, self.dim, len(self.radii)
        if dim not in (2, 3) or latent.shape[1] != dim:
            raise ValueError(f"GraphStore: coordinates of dimension 2 or 3 on both sides, got {dim} and {int(latent.shape[1])}")
        if S == 0 or N == 0 or Q == 0:
            raise ValueError("GraphStore: empty split, sample or latent grid")
        dev = x.device
        x = x.contiguous().float()
        latent = latent.contiguous().float()
        self.latent = latent                           # the shared token coordinates: what part_table()'s stride-0 column points at
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        self.x_scaled = _alloc(S, N, dim, dtype=torch.float32, device=dev)
        L.check(lib.gaot_rescale_batch(_p(x), S, N, dim, _p(self.x_scaled), _stream()), "gaot_rescale_batch")
        self.launches += LAUNCHES_RESCALE
        stats = _alloc(K, S, 3, **i64)
        for k, r in enumerate(self.radii):
            nb = int(lib.gaot_graph_store_scratch(S, N, Q, dim, r))
            if nb < 0:
                L.check(1, "gaot_graph_store_scratch")
            a = {"scratch": _alloc((nb + 7) // 8, **i64),
                 "enc_splits": _alloc(S, Q + 1, **i64), "dec_splits": _alloc(S, N + 1, **i64),
                 "enc_splits32": _alloc(S, Q + 1, **i32), "dec_splits32": _alloc(S, N + 1, **i32)}
            self._arenas.append(a)
            L.check(lib.gaot_graph_store_count(_p(self.x_scaled), S, N, _p(latent), Q, dim, r, _p(a["enc_splits"]), _p(a["dec_splits"]),
                                               _p(a["enc_splits32"]), _p(a["dec_splits32"]), _p(stats[k]), _p(a["scratch"]), _stream()),
                    "gaot_graph_store_count")
            self.launches += LAUNCHES_COUNT
        st = stats.cpu().numpy()                      # THE readback: (edges, longest encoder row, longest decoder row) per (scale, sample)
        self.edge_counts = torch.from_numpy(np.ascontiguousarray(st[:, :, 0].T))
        if int(st[:, :, 0].max()) >= (1 << 31):
            s_bad, k_bad = np.argwhere(st[:, :, 0].T >= (1 << 31))[0]
            raise ValueError(f"GraphStore: sample {int(s_bad)} has {int(st[k_bad, s_bad, 0])} edges at scale {int(k_bad)}: a single sample's "
                             "list must stay below 2^31 entries")
        for k, r in enumerate(self.radii):
            a = self._arenas[k]
            counts = st[k, :, 0]
            offs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
            total = int(offs[-1])
            max_row = int(max(st[k, :, 1].max(), st[k, :, 2].max()))
            a["offsets"] = torch.from_numpy(offs).to(dev)
            for name in ("enc_index", "dec_index"):
                a[name] = _alloc(total + 1, **i64)
            for name in ("enc_index32", "dec_index32", "enc_edge_query", "dec_edge_query", "enc_t_edge", "dec_t_edge"):
                a[name] = _alloc(total + 1, **i32)
            sort_scratch = _alloc(total, **i64) if max_row > 4096 else None
            L.check(lib.gaot_graph_store_fill(_p(self.x_scaled), S, N, _p(latent), Q, dim, r, _p(a["offsets"]), total, int(counts.max()), max_row,
                                              _p(a["enc_splits32"]), _p(a["dec_splits32"]), _p(a["enc_index"]), _p(a["dec_index"]),
                                              _p(a["enc_index32"]), _p(a["dec_index32"]), _p(a["enc_edge_query"]), _p(a["dec_edge_query"]),
                                              _p(a["enc_t_edge"]), _p(a["dec_t_edge"]), _p(a["scratch"]), _p(sort_scratch), _stream()),
                    "gaot_graph_store_fill")
            self.launches += LAUNCHES_FILL if total > 0 else 0
            del a["scratch"]                           # (stream-ordered: the allocator hands it out again only to later work of this stream)
            a["enc_deg"] = a["enc_splits"][:, 1:] - a["enc_splits"][:, :-1]
            a["dec_deg"] = a["dec_splits"][:, 1:] - a["dec_splits"][:, :-1]
            for s in range(S):
                b, E = int(offs[s]), int(counts[s])
                e1 = b + max(E, 1)                      # a plan's per-edge arrays have at least one entry, as GeometryPlan allocates them
                enc = {"neighbors_index": a["enc_index"][b:b + E], "neighbors_row_splits": a["enc_splits"][s]}
                dec = {"neighbors_index": a["dec_index"][b:b + E], "neighbors_row_splits": a["dec_splits"][s]}
                enc[P._PLAN_KEY] = P.GeometryPlan.from_arrays(
                    Q, E, N, a["enc_index32"][b:e1], a["enc_splits32"][s], a["enc_edge_query"][b:e1], a["dec_splits32"][s], a["enc_t_edge"][b:e1],
                    a["enc_deg"][s], st[k, s, 1], st[k, s, 2], index_long=enc["neighbors_index"], src_index=enc["neighbors_index"])
                dec[P._PLAN_KEY] = P.GeometryPlan.from_arrays(
                    N, E, Q, a["dec_index32"][b:e1], a["dec_splits32"][s], a["dec_edge_query"][b:e1], a["enc_splits32"][s], a["dec_t_edge"][b:e1],
                    a["dec_deg"][s], st[k, s, 2], st[k, s, 1], index_long=dec["neighbors_index"], src_index=dec["neighbors_index"])
                self.encoder[s].append(enc)
                self.decoder[s].append(dec)
        self.nbytes = self.x_scaled.numel() * 4 + sum(t.numel() * t.element_size() for a in self._arenas for t in a.values())

    def arenas(self, scale: int) -> dict:
        """the allocations behind scale `scale` of a device store (name -> tensor; per-sample entries offsets[s] .. offsets[s + 1])"""
        return self._arenas[scale]

    # ---- index-driven batches (plan.StaticUnion.bind_index, trainer.bind_samples): the whole split as ONE table per scale and side
    def part_table(self, scale: int, side: str) -> torch.Tensor:
        """device int64 [S, 8]: one gaot_union_part per sample -- the addresses of its plan arrays inside the arenas, its coordinates
        (`side` 'encoder': x_scaled[s] as sources, the shared latent grid with stride 0 as queries; 'decoder': the reverse) and its edge
        count in the high half of the last word (the low half, e_begin, depends on the batch: the indexed compose kernel takes the prefix
        sum itself).  Built once, vectorised on the host, one upload; the store must outlive whoever reads it.  Device stores only."""
        if side not in ("encoder", "decoder"):
            raise ValueError(f"GraphStore.part_table: side must be 'encoder' or 'decoder', got {side!r}")
        if not self._arenas:
            raise RuntimeError("GraphStore.part_table: a store built from host tensors has no device arenas to point into (build it from "
                               "device tensors; there is no fallback)")
        key = (int(scale), side)
        hit = self.__dict__.setdefault("_part_tables", {}).get(key)
        if hit is not None:
            return hit
        a = self._arenas[scale]
        S, N, Q = self.S, self.N, self.Q
        counts = self.edge_counts[:, scale].numpy().astype(np.int64)
        offs = np.concatenate(([0], np.cumsum(counts)[:-1])).astype(np.int64)
        s = np.arange(S, dtype=np.int64)
        pre, other, rows, t_rows = ("enc", "dec", Q, N) if side == "encoder" else ("dec", "enc", N, Q)
        tab = np.zeros((S, 8), dtype=np.int64)
        for col, name in enumerate((f"{pre}_index32", f"{pre}_edge_query", f"{pre}_t_edge")):
            tab[:, col] = a[name].data_ptr() + 4 * offs
        tab[:, 3] = a[f"{pre}_splits32"].data_ptr() + 4 * (rows + 1) * s
        tab[:, 4] = a[f"{other}_splits32"].data_ptr() + 4 * (t_rows + 1) * s
        x_ptr = self.x_scaled.data_ptr() + 4 * N * self.dim * s
        lat_ptr = np.full(S, self.latent.data_ptr(), dtype=np.int64)
        tab[:, 5], tab[:, 6] = (x_ptr, lat_ptr) if side == "encoder" else (lat_ptr, x_ptr)
        tab[:, 7] = counts << 32
        out = self._part_tables[key] = torch.from_numpy(tab).to(self.x_scaled.device)
        return out

    def batch_edge_capacity(self, B: int, scale: int) -> int:
        """edge capacity of the ONE static union that serves every batch of B samples of this split at `scale` (batch_edge_capacity below)"""
        return batch_edge_capacity(self.edge_counts[:, scale], B)


def batch_edge_capacity(counts, B: int) -> int:
    """plan.edge_bucket(sum of the B largest per-sample edge counts): any batch of B DISTINCT samples fits a union of this capacity, so one
    capacity -- one captured step -- serves the whole split whatever the shuffle.  B > S has no batch of distinct samples: an epoch's order
    then repeats the list (trainer.shard_indices), every sample at most ceil(B / S) times, and that is what is summed (the counts in
    descending order, cycled to B entries).  A list that repeats samples beyond that can exceed the capacity: the compose kernel flags it
    (status & 4) and truncates.  Capacities from 2^31 on are refused: the unions' edge ids are int32."""
    from .plan import edge_bucket
    c = np.sort(np.asarray(counts, dtype=np.int64).reshape(-1))[::-1]
    B = int(B)
    if B < 1 or c.size == 0:
        raise ValueError("batch_edge_capacity: needs at least one sample and a batch of at least one")
    total = int(c[np.arange(B) % c.size].sum())
    cap = edge_bucket(total)
    if cap >= (1 << 31):
        raise ValueError(f"batch_edge_capacity: a batch of {B} samples can hold {total} edges; a union's edge list must stay below 2^31 entries "
                         "(smaller batches, or a smaller radius)")
    return cap


class GraphBuilder:
    """The reference's GraphBuilder (src/datasets/graph_builder.py:13-144) over a GraphStore."""

    def __init__(self, neighbor_search_method: str = "auto"):
        if neighbor_search_method == "torch_cluster":
            raise NotImplementedError("GraphBuilder builds the exact uncapped graphs (" + ", ".join(_EXACT) + "); the capped, strict "
                                      "'torch_cluster' flavour is per sample: use NeighborSearch(method='torch_cluster')")
        if neighbor_search_method not in _EXACT:
            raise ValueError(f"unknown neighbor search method {neighbor_search_method!r}")
        self.method = neighbor_search_method

    def build_store(self, x_data: torch.Tensor, latent_queries: torch.Tensor, gno_radius: float, scales: List[float]) -> GraphStore:
        # the product in Python floats, narrowed to fp32 at the C boundary: what the reference hands NeighborSearch (graph_builder.py:65-67)
        return GraphStore(x_data, latent_queries, [float(gno_radius * s) for s in scales], self.method)

    def build_graphs_for_split(self, x_data: torch.Tensor, latent_queries: torch.Tensor, gno_radius: float, scales: List[float]) -> Tuple[List, List]:
        store = self.build_store(x_data, latent_queries, gno_radius, scales)
        return store.encoder, store.decoder

    def build_all_graphs(self, data_splits: dict, latent_queries: torch.Tensor, gno_radius: float, scales: List[float],
                         build_train: bool = True) -> dict:
        all_graphs = {}
        names = ["test"] + (["train", "val"] if build_train else [])
        for name in names:
            if name in data_splits:
                enc, dec = self.build_graphs_for_split(data_splits[name]["x"], latent_queries, gno_radius, scales)
                all_graphs[name] = {"encoder": enc, "decoder": dec}
        if not build_train:
            all_graphs["train"] = None
            all_graphs["val"] = None
        return all_graphs
