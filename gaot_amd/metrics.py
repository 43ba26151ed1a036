"""The reference's test metric on libgaot_hip.so (reference src/utils/metrics.py: `compute_batch_errors`, `compute_final_metric`):
the per-sample, per-variable-chunk relative L1 error, reduced by the median over samples and the mean over chunks.

Same two signatures, same semantics -- quirks included: the statistics and the chunk table are indexed through `active_variables` exactly
as metrics.py:24-33 does (CE-Gauss lists five chunk entries for four active variables), and a 3-D `[B, N, V]` input broadcasts against
the `[1, 1, 1, V]` statistics to `[1, B, N, V]`, so its result is ONE row pooled over the batch (what static_trainer.py:283-288 computes).
`metadata` is duck-typed: `active_variables`, `chunked_variables`, `global_mean`, `global_std`.

Device fp32 tensors only (no CPU fallback).  One streaming pass over both tensors and a small finishing launch per call; `denorm =
(mean, std)` folds the `data * std + mean` of trainer_utils.py:145 into that pass.  `ErrorLog` keeps the rows of a whole test set on the
device, so a test loop reads the host once.
"""
from typing import Optional, Tuple

import torch

from . import _lib as L
from .ops import _dev, _f32, _p, _stream

MAX_VARIABLES = 32          # csrc/metrics.hip REL_L1_MAX_V


class _Tables:
    """per-variable statistics and the chunk table of one metadata object on one device (metrics.py:24-36)"""

    def __init__(self, metadata, device):
        active = [int(i) for i in metadata.active_variables]
        gmean, gstd, orig = list(metadata.global_mean), list(metadata.global_std), list(metadata.chunked_variables)
        chunked = [orig[i] for i in active]
        unique = sorted(set(chunked))
        remap = {old: new for new, old in enumerate(unique)}
        self.V = len(active)
        self.C = len(unique)
        if not 1 <= self.V <= MAX_VARIABLES:
            raise ValueError(f"gaot_amd.metrics: {self.V} active variables; the kernel takes 1..{MAX_VARIABLES}")
        self.key = (tuple(active), tuple(float(gmean[i]) for i in active), tuple(float(gstd[i]) for i in active), tuple(chunked))
        self.mean = torch.tensor(self.key[1], dtype=torch.float32, device=device)
        self.std = torch.tensor(self.key[2], dtype=torch.float32, device=device)
        self.chunks = torch.tensor([remap[c] for c in chunked], dtype=torch.int32, device=device)


_TABLES: dict = {}


def _tables(metadata, device) -> _Tables:
    """cached by the metadata OBJECT (held, so its id stays unique) and re-validated by value: uploading three small tensors per batch
    would be three host-to-device copies in a loop that otherwise has none"""
    k = (id(metadata), device)
    hit = _TABLES.get(k)
    if hit is not None and hit[0] is metadata:
        active = [int(i) for i in metadata.active_variables]
        now = (tuple(active), tuple(float(metadata.global_mean[i]) for i in active), tuple(float(metadata.global_std[i]) for i in active),
               tuple(metadata.chunked_variables[i] for i in active))
        if now == hit[1].key:
            return hit[1]
    fresh = _Tables(metadata, device)
    if len(_TABLES) > 32:
        _TABLES.clear()
    _TABLES[k] = (metadata, fresh)
    return fresh


def _as_btnv(x: torch.Tensor, V: int, what: str) -> torch.Tensor:
    """[B, T, N, V] view the kernel can stride: inner [N, V] block contiguous, b / t strides >= N * V (a copy only where that fails)"""
    if x.dim() == 3:
        x = x.unsqueeze(0)              # the reference's broadcast against [1, 1, 1, V]: one pooled row
    if x.dim() != 4:
        raise ValueError(f"gaot_amd.metrics: `{what}` must be [B, T, N, V] (or [B, N, V]), got {tuple(x.shape)}")
    if x.shape[3] != V:
        raise ValueError(f"gaot_amd.metrics: `{what}` has {x.shape[3]} variables, metadata.active_variables lists {V}")
    if x.numel() == 0:
        raise ValueError(f"gaot_amd.metrics: `{what}` is empty")
    B, T, N, _ = x.shape
    S = N * V
    ok = (x.stride(3) == 1 and (N == 1 or x.stride(2) == V) and (T == 1 or x.stride(1) >= S) and (B == 1 or x.stride(0) >= S))
    return x if ok else x.contiguous()


def _denorm_tables(denorm, V: int, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    if denorm is None:
        return None, None
    mean, std = denorm
    out = []
    for t, name in ((std, "std"), (mean, "mean")):
        t = torch.as_tensor(t, dtype=torch.float32).to(device).reshape(-1)
        if t.numel() == 1:
            t = t.expand(V)
        if t.numel() != V:
            raise ValueError(f"gaot_amd.metrics: denorm {name} has {t.numel()} entries, expected {V} (or 1)")
        out.append(t.contiguous())
    return out[0], out[1]             # x * a + b with a = std, b = mean


def _launch(gtr, prd, tab: _Tables, denorm, out_rows: torch.Tensor) -> None:
    """rows of `out_rows` ([B, C] view with unit inner stride, any row stride) <- relative L1 errors of the batch"""
    lib = L.load()
    B, T, N, V = gtr.shape
    n_ws = int(lib.gaot_rel_l1_errors_workspace(B, T, N, V))
    if n_ws <= 0:
        raise L.GaotLibraryError(f"gaot_rel_l1_errors_workspace refused the shape {(B, T, N, V)}")
    ws = torch.empty(n_ws // 2, dtype=torch.float64, device=gtr.device)
    a, b = _denorm_tables(denorm, V, gtr.device)
    L.check(lib.gaot_rel_l1_errors(_p(gtr), gtr.stride(0), gtr.stride(1), _p(prd), prd.stride(0), prd.stride(1), B, T, N, V, _p(a), _p(b),
                                   _p(tab.mean), _p(tab.std), _p(tab.chunks), tab.C, _p(ws), _p(out_rows), out_rows.stride(0), _stream()),
            "gaot_rel_l1_errors")


def _prepare(gtr, prd, metadata):
    if not (torch.is_tensor(gtr) and torch.is_tensor(prd)):
        raise TypeError("gaot_amd.metrics takes torch tensors")
    _dev(gtr, prd)
    _f32(gtr, prd)
    if gtr.shape != prd.shape:
        raise ValueError(f"gaot_amd.metrics: ground truth {tuple(gtr.shape)} and prediction {tuple(prd.shape)} differ in shape")
    tab = _tables(metadata, gtr.device)
    return _as_btnv(gtr.detach(), tab.V, "gtr"), _as_btnv(prd.detach(), tab.V, "prd"), tab


def compute_batch_errors(gtr: torch.Tensor, prd: torch.Tensor, metadata, denorm=None) -> torch.Tensor:
    """relative L1 error per sample and variable chunk, [B, C] (metrics.py:11-58).  `denorm = (mean, std)`: both tensors are first
    de-normalised as `x * std + mean` (trainer_utils.py:145) inside the same pass."""
    g, p, tab = _prepare(gtr, prd, metadata)
    out = torch.empty(g.shape[0], tab.C, dtype=torch.float32, device=g.device)
    _launch(g, p, tab, denorm, out)
    return out


def _median_mean(rows: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(per-chunk lower medians [C], their mean as a 0-dim tensor) of rows [n, C] (unit inner stride, any row stride): device tensors"""
    n, C = rows.shape
    if n < 1:
        raise ValueError("gaot_amd.metrics: the median of no samples is undefined")
    med = torch.empty(C, dtype=torch.float32, device=rows.device)
    metric = torch.empty((), dtype=torch.float32, device=rows.device)
    L.check(L.load().gaot_median_mean(_p(rows), n, C, rows.stride(0) if n > 1 else max(rows.stride(0), C), _p(med), _p(metric), _stream()),
            "gaot_median_mean")
    return med, metric


def _rows(t: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError("gaot_amd.metrics takes torch tensors")
    _dev(t)
    _f32(t)
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"gaot_amd.metrics: expected [num_samples, num_chunks], got {tuple(t.shape)}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def chunk_medians(all_relative_errors: torch.Tensor) -> torch.Tensor:
    """the per-chunk lower medians over the samples, [C] on the device (what torch.median(dim=0)[0] returns, metrics.py:71)"""
    return _median_mean(_rows(all_relative_errors.detach()))[0]


def compute_final_metric(all_relative_errors: torch.Tensor) -> float:
    """median over the samples per chunk, mean over the chunks (metrics.py:60-76); the call's one host read is the returned float"""
    return float(_median_mean(_rows(all_relative_errors.detach()))[1].item())


class ErrorLog:
    """Device-resident `[capacity, C]` log of per-sample errors: `append` has the kernel write a batch's rows in place at an offset the
    host knows (no torch.cat, no host read), `final_metric()` is the run's single host read (static_trainer.py:274-292)."""

    def __init__(self, capacity: int, metadata, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("gaot_amd ops take device tensors only (no CPU fallback); got a host tensor")
        if capacity < 1:
            raise ValueError("ErrorLog: capacity must be positive")
        self.metadata = metadata
        self._tab = _tables(metadata, device)
        self.rows = torch.zeros(int(capacity), self._tab.C, dtype=torch.float32, device=device)
        self.count = 0

    def append(self, gtr: torch.Tensor, prd: torch.Tensor, denorm=None) -> torch.Tensor:
        g, p, tab = _prepare(gtr, prd, self.metadata)
        if g.device != self.rows.device:
            raise RuntimeError(f"ErrorLog lives on {self.rows.device}, the batch on {g.device}")
        B = g.shape[0]
        if self.count + B > self.rows.shape[0]:
            raise ValueError(f"ErrorLog: {self.count} + {B} rows exceed the capacity of {self.rows.shape[0]}")
        out = self.rows[self.count:self.count + B]
        _launch(g, p, tab, denorm, out)
        self.count += B
        return out

    def errors(self) -> torch.Tensor:
        return self.rows[:self.count]

    def final_metric(self) -> float:
        return compute_final_metric(self.errors())

    def reset(self) -> None:
        self.count = 0
