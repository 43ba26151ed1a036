"""The reference's test metric restated in plain torch, in our own words (any device, any float dtype): what tests/golden/eval_metrics.npz was
recorded from, and the yardstick for shapes too large for a fixture.

  normalise both fields with the statistics of the ACTIVE variables; per sample and variable, sum |truth - prediction| and |truth| over
  time and space; pool the variables of a chunk (chunk ids renumbered densely in sorted order); err = pooled error / (pooled truth + 1e-10).
  Final metric: the lower median over the samples per chunk (torch.median), then the mean over the chunks.
"""
import torch

EPS = 1e-10


def chunk_table(metadata):
    """(dense chunk id per active variable, number of chunks): the chunk list is indexed THROUGH the active variables -- CE-Gauss lists five
    chunk entries for four active variables, and only the entries the active variables point at count"""
    picked = [metadata.chunked_variables[i] for i in metadata.active_variables]
    dense = {c: k for k, c in enumerate(sorted(set(picked)))}
    return [dense[c] for c in picked], len(dense)


def batch_errors(gtr: torch.Tensor, prd: torch.Tensor, metadata) -> torch.Tensor:
    active = list(metadata.active_variables)
    mean = torch.tensor(metadata.global_mean, dtype=gtr.dtype, device=gtr.device)[active].reshape(1, 1, 1, -1)
    std = torch.tensor(metadata.global_std, dtype=gtr.dtype, device=gtr.device)[active].reshape(1, 1, 1, -1)
    chunks, C = chunk_table(metadata)
    g, p = (gtr - mean) / std, (prd - mean) / std          # a 3-D [B, N, V] input broadcasts to [1, B, N, V]: ONE pooled row
    per_var_err = (g - p).abs().sum(dim=(1, 2))
    per_var_ref = g.abs().sum(dim=(1, 2))
    num = torch.zeros(per_var_err.shape[0], C, dtype=gtr.dtype, device=gtr.device)
    den = torch.zeros_like(num)
    for v, c in enumerate(chunks):          # in variable order, like a serial scatter-add
        num[:, c] += per_var_err[:, v]
        den[:, c] += per_var_ref[:, v]
    return num / (den + EPS)


def final_metric(errs: torch.Tensor) -> float:
    return torch.median(errs, dim=0).values.mean().item()


class Meta:
    """duck-typed metadata: the four lists the metric reads"""

    def __init__(self, active, chunked, mean, std):
        self.active_variables = [int(i) for i in active]
        self.chunked_variables = [int(i) for i in chunked]
        self.global_mean = [float(x) for x in mean]
        self.global_std = [float(x) for x in std]


def load_fixture():
    """tests/golden/eval_metrics.npz -> {case: dict(gtr, prd, how, meta, ref32, ref64, d, [u_mean, u_std])}, plus the final-metric cases"""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz"))
    cases = {}
    for name in [str(s) for s in z["cases"]]:
        c = dict(gtr=torch.from_numpy(z[f"{name}/gtr"]), prd=torch.from_numpy(z[f"{name}/prd"]), how=str(z[f"{name}/how"]),
                 meta=Meta(z[f"{name}/active"], z[f"{name}/chunked"], z[f"{name}/global_mean"], z[f"{name}/global_std"]),
                 ref32=torch.from_numpy(z[f"{name}/ref32"]), ref64=torch.from_numpy(z[f"{name}/ref64"]), d=float(z[f"{name}/d"]))
        if c["how"] == "denorm":
            c["u_mean"], c["u_std"] = torch.from_numpy(z[f"{name}/u_mean"]), torch.from_numpy(z[f"{name}/u_std"])
        cases[name] = c
    finals = {tag: dict(errs=torch.from_numpy(z[f"{tag}/errs"]), ref32=float(z[f"{tag}/ref32"]), ref64=float(z[f"{tag}/ref64"]))
              for tag in ("final_n7", "final_n8")}
    return cases, finals


def reference_inputs(case, dtype):
    """the tensors the reference was handed for this case (a view of the stored fields, or their de-normalisation)"""
    g, p = case["gtr"].to(dtype), case["prd"].to(dtype)
    if case["how"] == "last_t":
        g, p = g[:, -1:], p[:, -1:]
    elif case["how"] == "denorm":
        m, s = case["u_mean"].to(dtype), case["u_std"].to(dtype)
        g, p = g * s + m, p * s + m
    return g, p
