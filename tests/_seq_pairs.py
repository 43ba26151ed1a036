"""tests/golden/seq_pairs.npz (the reference's DynamicPairDataset / TestDataset items, tests/golden/make_seq_pairs.py) as torch tensors,
loaded once and shared by tests/test_seq_pairs_cpu.py and tests/test_seq_pairs_gpu.py."""
import os

import numpy as np
import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_pairs.npz")


def load_fixture():
    z = np.load(PATH)
    data, cases = {}, {}
    for name in [str(n) for n in z["cases"]]:
        key = str(z[f"{name}/data"])
        if key not in data:
            stats = {}
            for k in z.files:
                if k.startswith(f"{key}/stats/"):
                    _, _, group, part = k.split("/")
                    v = z[k]
                    stats.setdefault(group, {})[part] = float(v) if v.ndim == 0 else torch.from_numpy(v)
            data[key] = dict(u=torch.from_numpy(z[f"{key}/u"]), c=torch.from_numpy(z[f"{key}/c"]) if f"{key}/c" in z.files else None,
                             t=torch.from_numpy(z[f"{key}/t"]), stats=stats)
        c = dict(data[key])
        c["kw"] = dict(max_time_diff=int(z[f"{name}/max_time_diff"]), time_step=int(z[f"{name}/time_step"]),
                       stepper_mode=str(z[f"{name}/stepper_mode"]), use_time_norm=bool(z[f"{name}/use_time_norm"]))
        for k in ("x", "y", "start_norm", "diff_norm", "time_diffs", "test_x0", "test_yseq"):
            c[k] = torch.from_numpy(z[f"{name}/{k}"])
        for k in ("t_in", "t_out", "test_time_indices"):
            c[k] = z[f"{name}/{k}"]
        cases[name] = c
    return cases


def make_store(case, device="cpu"):
    from gaot_amd.sequential import PairStore
    return PairStore(case["u"], case["c"], case["t"], case["stats"], device=device, **case["kw"])
