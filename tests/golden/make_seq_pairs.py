#!/usr/bin/env python3
"""Generate tests/golden/seq_pairs.npz by running the *imported reference* datasets (src/datasets/data_utils.py: DynamicPairDataset,
TestDataset) on small seeded trajectories.

Runs only where a checkout of the reference is at hand:  GAOT_REFERENCE_DIR=/path/to/reference python tests/golden/make_seq_pairs.py
(or the path as the first argument).  Data only is committed: this script and the arrays it wrote.

data_utils.py needs torch and numpy alone, so it is loaded BY FILE PATH (the reference's packages import xarray at package level).

Per case the fixture holds the seeded inputs (u, c, non-uniform t, the statistics, the hyper-parameters), the dataset's own pair tables,
`DynamicPairDataset[i]` for EVERY index i (input and target, stacked) and, for TestDataset over `test_time_indices`, every sample's x0 and
y_seq.  Cases: S=3 T=7 N=67 U=3 Cc=1 (N U and the row width odd) in the three stepper modes; S=2 T=5 N=1 U=1 without c and without time
normalisation; S=2 T=9 N=257 U=4 with time_step=1, max_time_diff=4 (T is truncated, data_utils.py:115-116).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref_dir):
    spec = importlib.util.spec_from_file_location("gaot_reference_data_utils", os.path.join(ref_dir, "src/datasets/data_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def trajectories(S, T, N, U, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    u_mean, u_std = torch.randn(U, generator=g), 0.5 + torch.rand(U, generator=g)
    # a drifting field: differences between time steps are well below the field itself, as in the datasets the steppers are made for
    base = u_mean + u_std * torch.randn(S, 1, N, U, generator=g)
    u = (base + 0.2 * u_std * torch.randn(S, T, N, U, generator=g).cumsum(dim=1)).contiguous()
    c = None
    stats = {"u": {"mean": u_mean, "std": u_std}}
    if Cc:
        c_mean, c_std = torch.randn(Cc, generator=g), 0.5 + torch.rand(Cc, generator=g)
        c = (c_mean + c_std * torch.randn(S, T, N, Cc, generator=g)).contiguous()
        stats["c"] = {"mean": c_mean, "std": c_std}
    t = (torch.arange(T, dtype=torch.float32) * 0.05 + 0.02 * torch.rand(T, generator=g)).contiguous()          # non-uniform, increasing
    stats["res"] = {"mean": 0.01 * torch.randn(U, generator=g), "std": 0.1 + 0.2 * torch.rand(U, generator=g)}
    stats["der"] = {"mean": 0.1 * torch.randn(U, generator=g), "std": 1.0 + torch.rand(U, generator=g)}
    stats["start_time"] = {"mean": 0.1375, "std": 0.0921}
    stats["time_diffs"] = {"mean": 0.1625, "std": 0.0713}
    return u, c, t, stats


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAOT_REFERENCE_DIR")
    if not ref_dir:
        raise SystemExit("usage: make_seq_pairs.py <reference checkout>   (or GAOT_REFERENCE_DIR)")
    D = load_reference(ref_dir)
    # name -> (data key, (S, T, N, U, Cc), seed, dataset keywords, TestDataset time indices)
    cases = {
        "n67_output": ("n67", (3, 7, 67, 3, 1), 1, dict(max_time_diff=6, time_step=2, stepper_mode="output", use_time_norm=True), [0, 2, 4, 6]),
        "n67_residual": ("n67", (3, 7, 67, 3, 1), 1, dict(max_time_diff=6, time_step=2, stepper_mode="residual", use_time_norm=True), [0, 2, 4, 6]),
        "n67_time_der": ("n67", (3, 7, 67, 3, 1), 1, dict(max_time_diff=6, time_step=2, stepper_mode="time_der", use_time_norm=True), [0, 2, 4, 6]),
        "n1_no_time_norm": ("n1", (2, 5, 1, 1, 0), 2, dict(max_time_diff=14, time_step=2, stepper_mode="output", use_time_norm=False), [0, 2, 4]),
        "n257_truncated": ("n257", (2, 9, 257, 4, 0), 3, dict(max_time_diff=4, time_step=1, stepper_mode="time_der", use_time_norm=True), [1, 2, 5, 8]),
    }
    out = {"cases": np.array(sorted(cases))}
    written = set()
    for name, (key, shape, seed, kw, tix) in sorted(cases.items()):
        u, c, t, stats = trajectories(*shape, seed)
        if key not in written:
            written.add(key)
            out[f"{key}/u"], out[f"{key}/t"] = u.numpy(), t.numpy()
            if c is not None:
                out[f"{key}/c"] = c.numpy()
            for k, v in stats.items():
                for part in ("mean", "std"):
                    out[f"{key}/stats/{k}/{part}"] = v[part].numpy() if torch.is_tensor(v[part]) else np.float64(v[part])
        ds = D.DynamicPairDataset(u, c, t, None, stats=stats, **kw)
        items = [ds[i] for i in range(len(ds))]
        x, y = D.collate_sequential_batch(items)
        assert x.dtype == torch.float32 and y.dtype == torch.float32
        out[f"{name}/data"] = np.array(key)
        for k, v in kw.items():
            out[f"{name}/{k}"] = np.array(v)
        out[f"{name}/x"], out[f"{name}/y"] = x.numpy(), y.numpy()
        out[f"{name}/t_in"], out[f"{name}/t_out"] = ds.t_in_indices.astype(np.int64), ds.t_out_indices.astype(np.int64)
        out[f"{name}/start_norm"], out[f"{name}/diff_norm"] = ds.start_times_norm.numpy(), ds.time_diffs_norm.numpy()
        out[f"{name}/time_diffs"] = ds.time_diffs.numpy()
        td = D.TestDataset(u, c, t, None, np.array(tix), stats)
        x0, yseq = zip(*[td[i] for i in range(len(td))])
        out[f"{name}/test_time_indices"] = np.array(tix, dtype=np.int64)
        out[f"{name}/test_x0"], out[f"{name}/test_yseq"] = torch.stack(x0).numpy(), torch.stack(yseq).numpy()
        print(f"{name:18s} S,T,N,U,Cc={shape}  pairs={len(ds.t_in_indices)}  items={len(ds)}  x {tuple(x.shape)}  y {tuple(y.shape)}")
    path = os.path.join(HERE, "seq_pairs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
