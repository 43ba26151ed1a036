#!/usr/bin/env python3
"""Generate tests/golden/graph_builder.npz by running the *imported reference* GraphBuilder (src/datasets/graph_builder.py, with
neighbor_search_method="grid") and rescale (src/utils/scaling.py) on small seeded point sets.

Runs only where a checkout of the reference is at hand:  GAOT_REFERENCE_DIR=/path/to/reference python tests/golden/make_graph_builder.py
(or the path as the first argument).  Data only is committed: this script and the arrays it wrote.

The reference's packages import xarray at package level (src/datasets/__init__.py); the three modules needed here (graph_builder.py,
neighbor_search.py, scaling.py) use torch alone, so they are loaded by file path under their own dotted names, with empty stand-ins for
the packages around them.

Cases (scales [1.0, 1.5] both):
  d2: three 2-D samples of 200 random points given as [S, N, d] -- sample 1 has a constant second coordinate (the zero-range branch of
      rescale) -- against a 7 x 7 latent grid, gno_radius 0.21;
  d3: two 3-D samples of 150 points given as [S, 1, N, d] against a 4 x 4 x 4 latent grid, gno_radius 0.45.
No (point, token) pair lies within 1e-5 relative of any radius (asserted in float64 on the rescaled coordinates), so the recorded lists do
not rest on how torch.norm rounds.  Per case the file holds the inputs, rescale's output per sample, and for every (sample, scale) the
index and row splits of both directions exactly as the reference returned them (the grid backend lists a row cell by cell).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = [1.0, 1.5]


def load_reference(ref_dir):
    for name in ("src", "src.datasets", "src.utils", "src.model", "src.model.layers", "src.model.layers.utils"):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = []
            sys.modules[name] = pkg
    mods = {}
    for name, rel in (("src.model.layers.utils.neighbor_search", "src/model/layers/utils/neighbor_search.py"),
                      ("src.utils.scaling", "src/utils/scaling.py"), ("src.datasets.graph_builder", "src/datasets/graph_builder.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_dir, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["src.datasets.graph_builder"], mods["src.utils.scaling"]


def grid(sizes):
    axes = [torch.linspace(-1.0, 1.0, n) for n in sizes]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, len(sizes)).contiguous()


def cases():
    g = torch.Generator().manual_seed(20)
    x2 = torch.rand(3, 200, 2, generator=g) * torch.tensor([3.0, 0.7]) + torch.tensor([-1.2, 4.0])          # far from [-1, 1]: rescale matters
    x2[1, :, 1] = 0.375
    x3 = (torch.randn(2, 1, 150, 3, generator=g) * torch.tensor([1.0, 0.5, 2.0])).contiguous()
    return {"d2": (x2.contiguous(), grid([7, 7]), 0.21), "d3": (x3, grid([4, 4, 4]), 0.45)}


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GAOT_REFERENCE_DIR")
    if not ref_dir:
        raise SystemExit("usage: make_graph_builder.py <reference checkout>   (or GAOT_REFERENCE_DIR)")
    GB, SC = load_reference(ref_dir)
    builder = GB.GraphBuilder(neighbor_search_method="grid")
    out = {"cases": np.array(sorted(cases())), "scales": np.array(SCALES, dtype=np.float64)}
    edges = 0
    for name, (x, lat, radius) in sorted(cases().items()):
        enc, dec = builder.build_graphs_for_split(x, lat, radius, SCALES)
        samples = x[:, 0] if x.dim() == 4 else x
        scaled = torch.stack([SC.rescale(s, (-1, 1)) for s in samples])
        assert scaled.dtype == torch.float32
        for k, sc in enumerate(SCALES):          # no pair near a radius: the lists do not depend on the rounding of the norm
            r = radius * sc
            d = (scaled.double()[:, :, None, :] - lat.double()[None, None, :, :]).norm(dim=-1)
            assert float(((d - r).abs() / r).min()) > 1e-5, (name, sc)
        out[f"{name}/x"], out[f"{name}/latent"], out[f"{name}/radius"] = x.numpy(), lat.numpy(), np.float64(radius)
        out[f"{name}/x_scaled"] = scaled.numpy()
        for s in range(samples.shape[0]):
            for k in range(len(SCALES)):
                for side, rows in (("enc", enc), ("dec", dec)):
                    idx, sp = rows[s][k]["neighbors_index"], rows[s][k]["neighbors_row_splits"]
                    assert idx.dtype == torch.int64 and sp.dtype == torch.int64
                    out[f"{name}/{side}/{s}/{k}/index"], out[f"{name}/{side}/{s}/{k}/splits"] = idx.numpy(), sp.numpy()
                edges += int(enc[s][k]["neighbors_index"].numel())
                assert enc[s][k]["neighbors_index"].numel() == dec[s][k]["neighbors_index"].numel()
        print(f"{name}: x {tuple(x.shape)} latent {tuple(lat.shape)} radius {radius} edges/sample/scale "
              f"{[[int(e['neighbors_index'].numel()) for e in row] for row in enc]}")
    assert 500 < edges < 6000, edges
    path = os.path.join(HERE, "graph_builder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", edges, "edges per direction")


if __name__ == "__main__":
    main()
