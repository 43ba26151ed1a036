#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics.npz by running the *imported reference* metric (src/utils/metrics.py) on small seeded cases.

Runs only where a checkout of the reference is at hand:  GAOT_REFERENCE_DIR=/path/to/reference python tests/golden/make_eval_metrics.py
(or the path as the first argument).  Data only is committed: this script and the arrays it wrote.

The reference's packages import xarray at package level (src/datasets/__init__.py), which the build container lacks; the two modules this
needs -- src/datasets/dataset.py (Metadata and the dataset table) and src/utils/metrics.py -- are plain torch, so they are loaded BY FILE
PATH with empty stand-in packages for `src`, `src.datasets` and `src.utils` in sys.modules.

Per case the fixture holds the inputs, the four metadata lists used, the reference's fp32 result, its float64 result (the same functions on
float64 inputs) and `d`: the largest relative distance between the two -- the reference's own rounding, on which the GPU test's bar is built
(|e - e64| <= (3 d + 2^-22) e64 per entry).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_reference(ref_dir):
    for name in ("src", "src.datasets", "src.utils"):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = []
            sys.modules[name] = pkg
    mods = {}
    for name, rel in (("src.datasets.dataset", "src/datasets/dataset.py"), ("src.utils.metrics", "src/utils/metrics.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_dir, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["src.datasets.dataset"], mods["src.utils.metrics"]


def meta(active, chunked, mean, std):
    return types.SimpleNamespace(active_variables=list(active), chunked_variables=list(chunked), global_mean=list(mean), global_std=list(std))


def fields(shape, mean, std, active, seed, noise=0.1):
    """ground truth spread like the data the statistics describe, prediction = truth + noise (a trained model's error level)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.tensor([mean[i] for i in active], dtype=torch.float32)
    s = torch.tensor([std[i] for i in active], dtype=torch.float32)
    gtr = m + s * torch.randn(*shape, generator=g)
    prd = gtr + noise * s * torch.randn(*shape, generator=g)
    return gtr.contiguous(), prd.contiguous()


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAOT_REFERENCE_DIR")
    if not ref_dir:
        raise SystemExit("usage: make_eval_metrics.py <reference checkout>   (or GAOT_REFERENCE_DIR)")
    D, M = load_reference(ref_dir)
    ce = D.DATASET_METADATA['compressible_flow/CE-Gauss']
    ce_lists = (ce.active_variables, ce.chunked_variables, ce.global_mean, ce.global_std)
    assert len(ce_lists[1]) == 5 and len(ce_lists[0]) == 4          # the quirk the fixture pins: five chunk entries, four active variables
    v1 = ([0], [0], [0.96086993], [0.18490477])
    v3 = ([0, 1, 2], [0, 1, 1], [0.8, 0.0, 2.513], [0.31, 0.391, 0.185])
    v5 = ([0, 1, 2, 3, 5], [0, 1, 1, 2, 3, 4], [0.80, 0., 0., 2.513, 9.0, 0.215], [0.31, 0.391, 0.356, 0.185, 1.0, 0.185])      # chunks [0,1,1,2,3]
    v2e = ([0, 1], [0, 1], [0.25, 0.5], [0.5, 0.25])          # exactly representable: a field equal to its mean normalises to 0 in fp32 AND float64
    # name -> (metadata lists, input shape, seed, how the reference is handed the inputs)
    cases = {
        "v1_n1": (v1, (1, 1, 1, 1), 1, "full"),
        "v3_n257_b5": (v3, (5, 1, 257, 3), 2, "full"),
        "v5_t3_b5": (v5, (5, 3, 257, 5), 3, "full"),
        "ce_gauss_last_t": (ce_lists, (5, 3, 257, 4), 4, "last_t"),          # sequential_trainer.py:433-434: y[:, -1:]
        "ce_gauss_pooled_3d": (ce_lists, (5, 257, 4), 5, "full"),            # static_trainer.py:283-288: [B, N, V] -> one pooled row
        "v2_truth_is_mean": (v2e, (2, 2, 64, 2), 6, "full"),
        "ce_gauss_denorm": (ce_lists, (2, 2, 64, 4), 7, "denorm"),
    }
    out = {"cases": np.array(sorted(cases))}
    for name, (lists, shape, seed, how) in sorted(cases.items()):
        md = meta(*lists)
        gtr, prd = fields(shape, lists[2], lists[3], lists[0], seed)
        if name == "v2_truth_is_mean":
            gtr[..., 1] = 0.5
        res = {}
        for dt in (torch.float32, torch.float64):
            g, p = gtr.to(dt), prd.to(dt)
            if how == "last_t":
                g, p = g[:, -1:], p[:, -1:]
            if how == "denorm":          # the inputs are NORMALISED fields; trainer_utils.py:145 in front of the metric
                g0 = torch.Generator().manual_seed(seed + 100)
                u_mean = torch.tensor([lists[2][i] for i in lists[0]], dtype=torch.float32) + 0.01 * torch.randn(len(lists[0]), generator=g0)
                u_std = torch.tensor([lists[3][i] for i in lists[0]], dtype=torch.float32) * (1 + 0.05 * torch.rand(len(lists[0]), generator=g0))
                if dt == torch.float32:
                    gtr = (gtr - u_mean) / u_std
                    prd = (prd - u_mean) / u_std
                    out[f"{name}/u_mean"], out[f"{name}/u_std"] = u_mean.numpy(), u_std.numpy()
                g, p = gtr.to(dt) * u_std.to(dt) + u_mean.to(dt), prd.to(dt) * u_std.to(dt) + u_mean.to(dt)
            res[dt] = M.compute_batch_errors(g, p, md)
        e32, e64 = res[torch.float32], res[torch.float64]
        d = float(((e32.double() - e64).abs() / e64.abs()).max())
        out[f"{name}/gtr"], out[f"{name}/prd"] = gtr.numpy(), prd.numpy()
        out[f"{name}/how"] = np.array(how)
        out[f"{name}/active"] = np.array(lists[0], dtype=np.int64)
        out[f"{name}/chunked"] = np.array(lists[1], dtype=np.int64)
        out[f"{name}/global_mean"] = np.array(lists[2], dtype=np.float64)
        out[f"{name}/global_std"] = np.array(lists[3], dtype=np.float64)
        out[f"{name}/ref32"], out[f"{name}/ref64"], out[f"{name}/d"] = e32.numpy(), e64.numpy(), np.float64(d)
        print(f"{name:22s} {str(tuple(shape)):18s} -> {tuple(e32.shape)}  d = {d:.2e}")
    # compute_final_metric: odd and even sample counts (lower median), ties
    g = torch.Generator().manual_seed(11)
    for tag, n in (("final_n7", 7), ("final_n8", 8)):
        errs = torch.rand(n, 3, generator=g) * 0.1
        errs[1, 0] = errs[4, 0]
        out[f"{tag}/errs"] = errs.numpy()
        out[f"{tag}/ref32"] = np.float64(M.compute_final_metric(errs))
        out[f"{tag}/ref64"] = np.float64(M.compute_final_metric(errs.double()))
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
    print("wrote", os.path.join(HERE, "eval_metrics.npz"))


if __name__ == "__main__":
    main()
