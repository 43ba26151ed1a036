"""Static (time-independent) training fed from the device: the reference's static datasets (src/datasets/data_utils.py, the loop of
static_trainer.py:160-202) as a resident store and ONE gather launch per batch.

The reference takes c[i], u[i] and -- variable coordinates (vx) -- the rescaled coordinates and the per-sample graphs of every item on
the host, collates them and uploads the batch, once per step.  A `SampleStore` keeps c and u (already normalised, as the reference's data
processor leaves them) on the device; for vx it sits on top of a device `graphs.GraphStore`, which holds the rescaled coordinates and every
sample's graphs.  A batch is a DEVICE list of B sample indices: `compose` copies the B blocks in one launch (csrc/sample_store.hip) and the
unions of the batch's graphs are composed from the same list (plan.StaticUnion.bind_index).  The list is the only thing that changes
between steps and it is not a launch argument, so all of it sits inside a captured step (`TrainStep.bind_samples` / `EvalStep.bind_samples`):

    store = GraphBuilder().build_store(x_train.cuda(), latent, radius, scales)
    data  = SampleStore(c_data, u_data, graphs=store)                 # vx; fx: SampleStore(c_data, u_data, coord=coord)
    ts.bind_samples(data, batch_size=B, latent_tokens_coord=latent)
    order = data.epoch_indices(epoch, rank, world)                    # device int32, uploaded once per epoch
    for k in range(len(data) // B):
        loss = ts.step_samples(order[k * B:(k + 1) * B])

The gather is a pure copy: what lands in the step's buffers equals c[idx], u[idx], x_scaled[idx] bit for bit.  On a CPU store the same
buffers are filled by torch indexing (the gloo tests of the data-parallel plumbing, a host loop); vx needs a device GraphStore.
"""
from typing import Optional

import torch


class SampleStore:
    """c [S, N, Cc] and u [S, N, U] of a static dataset on `device`, with the geometry they live on: `graphs` (a device graphs.GraphStore:
    vx, every sample its own coordinates and graphs) or `coord` ([N, d]: fx, one mesh for all samples).  `len(store)` = S."""

    def __init__(self, c_data: Optional[torch.Tensor], u_data: torch.Tensor, graphs=None, coord: Optional[torch.Tensor] = None, device=None):
        if c_data is None:
            raise ValueError("SampleStore: c_data is required -- the model's input is c (a dataset without condition fields feeds its "
                             "coordinates as c, as the reference's data processor does); got None")
        for name, t in (("c_data", c_data), ("u_data", u_data)):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3:
                raise ValueError(f"SampleStore: {name} must be an fp32 tensor [S, N, channels], got {getattr(t, 'dtype', type(t))} "
                                 f"{tuple(getattr(t, 'shape', ()))}")
        if c_data.shape[0] != u_data.shape[0]:
            raise ValueError(f"SampleStore: c_data holds {int(c_data.shape[0])} samples, u_data {int(u_data.shape[0])}")
        if c_data.shape[1] != u_data.shape[1]:
            raise ValueError(f"SampleStore: c_data has {int(c_data.shape[1])} nodes per sample, u_data {int(u_data.shape[1])}")
        if min(c_data.shape) == 0 or min(u_data.shape) == 0:
            raise ValueError("SampleStore: empty dataset, sample or channel axis")
        if (graphs is None) == (coord is None):
            raise ValueError("SampleStore: give exactly one of graphs= (vx: a device GraphStore) and coord= (fx: the shared [N, d] mesh)")
        self.S, self.N, self.Cc = (int(v) for v in c_data.shape)
        self.U = int(u_data.shape[2])
        self.graphs = graphs
        if graphs is not None:
            if not getattr(graphs, "x_scaled", torch.empty(0)).is_cuda:
                raise RuntimeError("SampleStore: vx needs a GraphStore built from device tensors (the batch's unions are composed from its "
                                   "device arenas; there is no host path)")
            if graphs.S != self.S or graphs.N != self.N:
                raise ValueError(f"SampleStore: the GraphStore holds {graphs.S} samples of {graphs.N} nodes, the data {self.S} of {self.N}")
            dev = graphs.x_scaled.device
            if device is not None and torch.device(device).type != dev.type:
                raise ValueError(f"SampleStore: device={device!r} but the GraphStore lives on {dev}")
            self.device = dev
            self.coord = None
            self.x_scaled = graphs.x_scaled
        else:
            if not torch.is_tensor(coord) or coord.dtype != torch.float32 or coord.dim() != 2 or coord.shape[0] != self.N:
                raise ValueError(f"SampleStore: coord must be an fp32 tensor [{self.N}, d]")
            self.device = torch.device(device) if device is not None else u_data.device
            self.coord = coord.detach().to(self.device).contiguous()
            self.x_scaled = None
        if self.N * max(self.Cc, self.U, 0 if graphs is None else graphs.dim) >= 2 ** 31:
            raise ValueError("SampleStore: one sample's [N, channels] block must stay below 2^31 elements")
        f32 = dict(dtype=torch.float32, device=self.device)
        self.c = c_data.detach().to(**f32).contiguous()
        self.u = u_data.detach().to(**f32).contiguous()
        self._flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._unions = []             # vx: the unions bound to this store's tables (their flags are part of status())

    @property
    def vx(self) -> bool:
        return self.graphs is not None

    def __len__(self) -> int:
        return self.S

    def epoch_indices(self, epoch: int, rank: int = 0, world: int = 1, shuffle: bool = True, seed: int = 0) -> torch.Tensor:
        """this rank's share of one epoch's sample order as a device int32 list (trainer.shard_indices over len(store): every rank derives
        the same permutation, padded to a multiple of `world`, strided) -- uploaded once per epoch; slices of it go to step_samples()"""
        from .trainer import shard_indices
        return torch.tensor(shard_indices(len(self), rank, world, epoch, shuffle, seed), dtype=torch.int32, device=self.device)

    def compose(self, idx: torch.Tensor, x: torch.Tensor, y: torch.Tensor, xcoord: Optional[torch.Tensor] = None) -> None:
        """x [B, N, Cc] <- c[idx], y [B, N, U] <- u[idx] and -- vx -- xcoord [B, N, d] <- x_scaled[idx] for the device int32 list idx [B]:
        one launch on the GPU (capturable; an index outside [0, len(store)) is clamped and flagged, status()), torch indexing on a CPU
        store (which raises for such an index)."""
        B = int(idx.numel())
        if self.vx != (xcoord is not None):
            raise ValueError("SampleStore.compose: xcoord goes with a vx store (graphs=), and only with one")
        want = [("idx", idx, (B,), torch.int32), ("x", x, (B, self.N, self.Cc), torch.float32), ("y", y, (B, self.N, self.U), torch.float32)]
        if xcoord is not None:
            want.append(("xcoord", xcoord, (B, self.N, self.graphs.dim), torch.float32))
        for name, t, shape, dt in want:
            if t.device != self.c.device or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"SampleStore.compose: {name} must be a contiguous {dt} tensor of shape {shape} on {self.c.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if self.device.type != "cuda":
            i = idx.long()
            if B and (int(i.min()) < 0 or int(i.max()) >= self.S):
                raise IndexError(f"SampleStore: index outside [0, {self.S})")
            x.copy_(self.c[i])
            y.copy_(self.u[i])
            return
        from . import _lib as L
        from .ops import _p, _stream
        L.check(L.load().gaot_sample_gather(_p(self.c), _p(self.u), _p(self.x_scaled), self.S, self.N, self.Cc, self.U,
                                            self.graphs.dim if self.vx else 0, _p(idx), B, _p(x), _p(y), _p(xcoord), _p(self._flag), _stream()),
                "gaot_sample_gather")

    def status(self) -> int:
        """what the launches OR-ed together since the last clear_status() (1: a sample index was out of range and clamped; 4: a batch's
        graphs -- a list that repeats samples -- exceeded a union's edge capacity and were truncated); synchronises"""
        self._unions = [r for r in self._unions if r() is not None]
        unions = [u for u in (r() for r in self._unions) if u is not None]
        out = 0
        for v in torch.cat([self._flag] + [u.flag for u in unions]).tolist():          # (one transfer)
            out |= int(v)
        return out

    def clear_status(self) -> None:
        self._flag.zero_()
        for r in self._unions:
            if r() is not None:
                r().flag.zero_()

    def _watch(self, unions) -> None:
        """unions composed from this store's tables (trainer.bind_samples): their status words are read with the store's"""
        import weakref
        self._unions.extend(weakref.ref(u) for u in unions)
