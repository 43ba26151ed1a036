"""Sequential (time-dependent) training fed from the device: the reference's `DynamicPairDataset` and `TestDataset`
(src/datasets/data_utils.py:73-235, 317-402) as ONE launch per batch over trajectories that stay resident.

The reference builds every training item on the CPU -- pick (sample, t_in, t_out), normalise u and c, append two time columns, form
the target by stepper mode -- then collates and copies the batch to the device, once per step.  The trajectories are small next to the
card's memory (1 024 samples x 21 steps x 16 384 nodes x 4 channels: 5.6 GB), so a `PairStore` keeps them there and composes a batch
from a DEVICE list of B flat dataset indices (csrc/seq_pairs.hip).  The list is the only thing that changes between steps and it is
not a launch argument, so the composition sits inside a captured training step (`TrainStep.bind_pairs` / `EvalStep.bind_pairs`).

Bit equality: the per-pair time features are built on the host with the reference's own torch fp32 expressions, and the kernel rounds
every operation on its own in the reference's order; what `store.batch(idx)` returns equals `collate_sequential_batch([dataset[i] for i
in idx])` bit for bit (tests/golden/seq_pairs.npz).  fx geometry only: vx sequential training needs a graph per (sample, time step).
"""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

MODES = {"output": 0, "residual": 1, "time_der": 2}


def time_pairs(num_timesteps: int, time_step: int) -> Tuple[np.ndarray, np.ndarray]:
    """the (t_in, t_out) index pairs in the reference's order (data_utils.py:121-135): lags time_step, 2 time_step, ... <= num_timesteps,
    for each lag every start 0, time_step, ... that fits.  `num_timesteps` is the count AFTER the truncation min(T - 1, max_time_diff)."""
    t_in, t_out = [], []
    for lag in range(time_step, num_timesteps + 1, time_step):
        for i in range(0, num_timesteps - lag + 1, time_step):
            t_in.append(i)
            t_out.append(i + lag)
    return np.array(t_in, dtype=np.int64), np.array(t_out, dtype=np.int64)


def _host(v):
    return v.detach().cpu() if torch.is_tensor(v) else v


class PairStore:
    """The trajectories of a time-dependent dataset on `device` plus the per-pair tables of DynamicPairDataset.

        store = PairStore(u_data, c_data, t_values, stats, max_time_diff=14, time_step=2, stepper_mode="time_der", device="cuda")
        x, y = store.batch(idx)                       # == collate_sequential_batch([dataset[i] for i in idx]), bit for bit
        order = store.epoch_indices(epoch, rank, world)          # device int32, uploaded once per epoch
        step.bind_pairs(store, B, ...); step.step_pairs(order[k * B:(k + 1) * B])

    u_data [S, T, N, U] and c_data [S, T, N, Cc] (or None) and t_values [T] are fp32 tensors; `stats` is the reference's dictionary
    ("u", optional "c", "start_time" / "time_diffs" when use_time_norm, "res" / "der" for the residual / time_der stepper).  `len(store)`
    = S * n_pairs; index i is sample i // n_pairs, pair i % n_pairs (data_utils.py:169-170).  On a CPU store the same results come from
    plain torch expressions (`batch_torch`); on the GPU everything goes through the kernels -- a missing library is an error."""

    def __init__(self, u_data: torch.Tensor, c_data: Optional[torch.Tensor], t_values: torch.Tensor, stats: Optional[dict],
                 max_time_diff: int = 14, time_step: int = 2, stepper_mode: str = "output", use_time_norm: bool = True, device=None):
        if stepper_mode not in MODES:
            raise ValueError(f"Unsupported stepper_mode: {stepper_mode}")
        if stats is None or "u" not in stats:
            raise ValueError("PairStore: stats with a 'u' entry are required (the 'output' target and the inputs are normalised by them)")
        need = {"residual": ["res"], "time_der": ["der"]}.get(stepper_mode, []) + (["start_time", "time_diffs"] if use_time_norm else [])
        missing = [k for k in need if k not in stats]
        if missing:
            raise ValueError(f"PairStore: stats lack {missing} (stepper_mode={stepper_mode!r}, use_time_norm={use_time_norm})")
        t_values = torch.as_tensor(t_values)
        for name, t in (("u_data", u_data), ("c_data", c_data), ("t_values", t_values)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32):
                raise ValueError(f"PairStore: {name} must be an fp32 tensor, got {getattr(t, 'dtype', type(t))}")
        if u_data.dim() != 4 or t_values.dim() != 1 or t_values.shape[0] != u_data.shape[1]:
            raise ValueError("PairStore: u_data must be [S, T, N, U] and t_values [T]")
        if c_data is not None and (c_data.dim() != 4 or c_data.shape[:3] != u_data.shape[:3]):
            raise ValueError("PairStore: c_data must be [S, T, N, Cc] with u_data's S, T, N")
        if int(time_step) < 1:
            raise ValueError("PairStore: time_step must be at least 1")
        self.device = torch.device(device) if device is not None else u_data.device
        self.S, self.T, self.N, self.U = (int(v) for v in u_data.shape)
        self.Cc = 0 if c_data is None else int(c_data.shape[3])
        self.stepper_mode, self.mode = stepper_mode, MODES[stepper_mode]
        self.use_time_norm = bool(use_time_norm)
        self.stats = stats
        # ---- the pair tables, on the host, by the reference's expressions (data_utils.py:115-147)
        self.num_timesteps = min(self.T - 1, int(max_time_diff))
        self.t_values = t_values.detach().cpu()[:self.num_timesteps + 1]
        self.t_in, self.t_out = time_pairs(self.num_timesteps, int(time_step))
        if len(self.t_in) == 0:
            raise ValueError(f"PairStore: no time pair fits (T={self.T}, max_time_diff={max_time_diff}, time_step={time_step})")
        self.time_diffs = self.t_values[self.t_out] - self.t_values[self.t_in]
        if self.use_time_norm:
            start_times = self.t_values[self.t_in]
            self.start_times_norm = (start_times - _host(stats["start_time"]["mean"])) / _host(stats["start_time"]["std"])
            self.time_diffs_norm = (self.time_diffs - _host(stats["time_diffs"]["mean"])) / _host(stats["time_diffs"]["std"])
        else:
            self.start_times_norm = self.t_values[self.t_in]
            self.time_diffs_norm = self.time_diffs
        for t in (self.time_diffs, self.start_times_norm, self.time_diffs_norm):
            if t.dtype != torch.float32:
                raise ValueError(f"PairStore: the time statistics promote the fp32 time features to {t.dtype}; give them as Python numbers or fp32")
        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.u = u_data.detach().to(**f32).contiguous()
        self.c = None if c_data is None else c_data.detach().to(**f32).contiguous()
        self._t_in = torch.tensor(self.t_in, dtype=torch.int32, device=dev)
        self._t_out = torch.tensor(self.t_out, dtype=torch.int32, device=dev)
        self._start_norm = self.start_times_norm.to(**f32).contiguous()
        self._diff_norm = self.time_diffs_norm.to(**f32).contiguous()
        self._diff = self.time_diffs.to(**f32).contiguous()
        self._u_mean, self._u_std = self._per_channel("u", self.U)
        self._c_mean, self._c_std = self._per_channel("c", self.Cc) if (self.Cc and "c" in stats) else (None, None)
        akey = {1: "res", 2: "der"}.get(self.mode)
        self._a_mean, self._a_std = self._per_channel(akey, self.U) if akey else (None, None)
        self._flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.S * self.n_pairs >= 2 ** 31 or self.N * (self.U + self.Cc + 2) >= 2 ** 31:
            raise ValueError("PairStore: S * n_pairs and N * (U + Cc + 2) must stay below 2^31")

    def _per_channel(self, key: str, width: int):
        """[width] fp32 mean / std on the device: scalars and [1] broadcast as the reference's expression would"""
        out = []
        for part in ("mean", "std"):
            t = torch.as_tensor(self.stats[key][part]).detach().to(dtype=torch.float32, device=self.device).reshape(-1)
            if t.numel() == 1:
                t = t.expand(width)
            if t.numel() != width:
                raise ValueError(f"PairStore: stats['{key}']['{part}'] has {t.numel()} entries, expected {width} (or 1)")
            out.append(t.contiguous())
        return out

    # ---- sizes
    @property
    def n_pairs(self) -> int:
        return len(self.t_in)

    def __len__(self) -> int:
        return self.S * self.n_pairs

    def input_width(self, conditional_norm: bool = False) -> int:
        """columns of a composed input: u, c, the start time and -- unless the model is fed the time through `condition` -- the time difference"""
        return self.U + self.Cc + (1 if conditional_norm else 2)

    # ---- indices
    def _index_tensor(self, idx) -> torch.Tensor:
        if torch.is_tensor(idx):
            return idx.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        return torch.tensor([int(i) for i in idx], dtype=torch.int32, device=self.device)

    def epoch_indices(self, epoch: int, rank: int = 0, world: int = 1, shuffle: bool = True, seed: int = 0) -> torch.Tensor:
        """this rank's share of one epoch's item order as a device int32 list (trainer.shard_indices over len(store): every rank derives
        the same permutation, padded to a multiple of `world`, strided) -- uploaded once per epoch; slices of it go to step_pairs()"""
        from .trainer import shard_indices
        return torch.tensor(shard_indices(len(self), rank, world, epoch, shuffle, seed), dtype=torch.int32, device=self.device)

    # ---- the launch
    def compose(self, idx: torch.Tensor, x_out: torch.Tensor, y_out: torch.Tensor, cond_out: Optional[torch.Tensor] = None) -> None:
        """x_out [B, N, U + Cc + 2] (with cond_out [B] or [B, 1]: [B, N, U + Cc + 1]), y_out [B, N, U] <- the items idx [B] (device int32):
        one launch, capturable.  Indices outside [0, len(store)) are clamped and flagged (status())."""
        from . import _lib as L
        from .ops import _p, _stream
        if self.device.type != "cuda":
            raise RuntimeError("gaot_amd ops take device tensors only (no CPU fallback); PairStore.compose needs a store on the GPU (batch_torch serves a CPU store)")
        B = int(idx.numel())
        n_time = 2 if cond_out is None else 1
        W = self.U + self.Cc + n_time
        for name, t, shape, dt in (("idx", idx, (B,), torch.int32), ("x_out", x_out, (B, self.N, W), torch.float32),
                                   ("y_out", y_out, (B, self.N, self.U), torch.float32)):
            if t.device != self.u.device or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"PairStore.compose: {name} must be a contiguous {dt} tensor of shape {shape} on {self.u.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
        if cond_out is not None and (cond_out.device != self.u.device or cond_out.dtype != torch.float32 or cond_out.numel() != B
                                     or not cond_out.is_contiguous()):
            raise ValueError(f"PairStore.compose: cond_out must be a contiguous fp32 tensor of {B} entries on {self.u.device}")
        L.check(L.load().gaot_seq_pairs_compose(
            _p(self.u), _p(self.c), self.S, self.T, self.N, self.U, self.Cc, _p(self._t_in), _p(self._t_out), _p(self._start_norm),
            _p(self._diff_norm), _p(self._diff), self.n_pairs, _p(self._u_mean), _p(self._u_std), _p(self._c_mean), _p(self._c_std),
            _p(self._a_mean), _p(self._a_std), self.mode, n_time, _p(idx), B, _p(x_out), _p(y_out), _p(cond_out), _p(self._flag), _stream()),
            "gaot_seq_pairs_compose")

    def status(self) -> int:
        """the flag the launches OR into (1: a dataset / sample index was out of range and clamped; 2: a time index was); synchronises"""
        return int(self._flag.item())

    def clear_status(self) -> None:
        self._flag.zero_()

    def batch(self, idx, conditional_norm: bool = False):
        """allocating convenience: (x, y) -- with conditional_norm (x[..., :-1], y, condition [B, 1]) -- for a list or tensor of indices"""
        if self.device.type != "cuda":
            return self.batch_torch(idx, conditional_norm)
        idx = self._index_tensor(idx)
        B = int(idx.numel())
        x = torch.empty(B, self.N, self.input_width(conditional_norm), dtype=torch.float32, device=self.device)
        y = torch.empty(B, self.N, self.U, dtype=torch.float32, device=self.device)
        cond = torch.empty(B, 1, dtype=torch.float32, device=self.device) if conditional_norm else None
        self.compose(idx, x, y, cond)
        return (x, y, cond) if conditional_norm else (x, y)

    def batch_torch(self, idx, conditional_norm: bool = False, check: bool = True):
        """the same batch by plain torch expressions on the store's device (data_utils.py:162-235 over a batch): what a CPU store
        answers with, and the baseline tools/seq_pairs_bench.py times the kernel against.  Indices must be in range (`check`: verified
        here, which on a GPU store reads the host; torch's indexing does not clamp)."""
        idx = self._index_tensor(idx).long()
        if check and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(self)):
            raise IndexError(f"PairStore: index outside [0, {len(self)})")
        s, p = idx // self.n_pairs, idx % self.n_pairs
        ti, to = self._t_in.long()[p], self._t_out.long()[p]
        u_in, u_out = self.u[s, ti], self.u[s, to]
        cols = [(u_in - self._u_mean) / self._u_std]
        if self.c is not None:
            c_in = self.c[s, ti]
            cols.append((c_in - self._c_mean) / self._c_std if self._c_mean is not None else c_in)
        B = idx.numel()
        cols.append(self._start_norm[p].view(B, 1, 1).expand(B, self.N, 1))
        if not conditional_norm:
            cols.append(self._diff_norm[p].view(B, 1, 1).expand(B, self.N, 1))
        x = torch.cat(cols, dim=-1)
        if self.mode == 0:
            y = (u_out - self._u_mean) / self._u_std
        elif self.mode == 1:
            y = (u_out - u_in - self._a_mean) / self._a_std
        else:
            y = ((u_out - u_in) / self._diff[p].view(B, 1, 1) - self._a_mean) / self._a_std
        return (x, y, self._start_norm[p].view(B, 1).clone()) if conditional_norm else (x, y)

    # ---- the test loop's items (TestDataset, data_utils.py:355-402)
    def test_batch(self, sample_ids, time_indices: Sequence[int]):
        """(x0 [B, N, U + Cc + 2], y_seq [B, K, N, U]) for the samples `sample_ids` and the K + 1 time indices of a rollout: the normalised
        state at time_indices[0] with two zero time columns (autoregressive_predict fills them per step) and the fields as stored at
        time_indices[1:] -- ready for `model.autoregressive_predict` and `metrics.ErrorLog`"""
        tix = [int(t) for t in np.asarray(time_indices).reshape(-1)]
        if len(tix) < 1:
            raise ValueError("PairStore.test_batch: time_indices is empty")
        K = len(tix) - 1
        if self.device.type != "cuda":
            if min(tix) < 0 or max(tix) >= self.T:
                raise IndexError(f"PairStore.test_batch: time index outside [0, {self.T})")
            s = self._index_tensor(sample_ids).long()
            u0 = self.u[s, tix[0]]
            cols = [(u0 - self._u_mean) / self._u_std]
            if self.c is not None:
                c0 = self.c[s, tix[0]]
                cols.append((c0 - self._c_mean) / self._c_std if self._c_mean is not None else c0)
            zero = torch.zeros(s.numel(), self.N, 1, dtype=torch.float32)
            return torch.cat(cols + [zero, zero], dim=-1), self.u[s][:, tix[1:]]
        from . import _lib as L
        from .ops import _p, _stream
        idx = self._index_tensor(sample_ids)
        B = int(idx.numel())
        tidx = torch.tensor(tix, dtype=torch.int32, device=self.device)
        x0 = torch.empty(B, self.N, self.U + self.Cc + 2, dtype=torch.float32, device=self.device)
        yseq = torch.empty(B, K, self.N, self.U, dtype=torch.float32, device=self.device)
        L.check(L.load().gaot_seq_test_compose(_p(self.u), _p(self.c), self.S, self.T, self.N, self.U, self.Cc, _p(self._u_mean), _p(self._u_std),
                                               _p(self._c_mean), _p(self._c_std), _p(idx), B, _p(tidx), K, _p(x0), _p(yseq) if K else None,
                                               _p(self._flag), _stream()), "gaot_seq_test_compose")
        return x0, yseq
