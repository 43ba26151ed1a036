#!/usr/bin/env python3
"""The three grouped helper launches of the bench step (gaot_absmax_grouped, gaot_split_f16_planes_grouped, gaot_colsum_grouped) on
their own: one eager step of the bench configuration records the item tables the step hands them, then the same tables are launched
on buffers of this tool's, `reps` times per value of gaot_debug_set_grouped_helpers, in alternation.
    python tools/grouped_helpers_bench.py [reps] [values ...]          (default: 50 repetitions of 0 and 7)
Prints the tables' shapes and device-event times per launch.  Under `rocprofv3 --kernel-trace` (or a --pmc pass of its own) the two
forms of each kernel are told apart by their template argument; the bench model's own launches come first in the trace."""
import collections, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import torch
import bench
from gaot_amd import ops, _lib as L
from gaot_amd.trainer import TrainStep

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
values = [int(v) for v in sys.argv[2:]] or [0, 7]
lib = L.load()
dev = torch.device("cuda:0")
tables = {"gaot_absmax_grouped": [], "gaot_split_f16_planes_grouped": [], "gaot_colsum_grouped": []}


def recorder(name, fn):
    def call(arr, n, stream):
        if not tables[name] or n > len(tables[name]):          # the largest call of the step: the weight table / the end-of-backward queue
            tables[name] = [tuple(getattr(arr[i], f) for f, _ in arr[i]._fields_) for i in range(n)]
        return fn(arr, n, stream)
    return call


real = {k: getattr(lib, k) for k in tables}
for k in tables:
    setattr(lib, k, recorder(k, real[k]))
torch.manual_seed(0)
model = bench.build_model().to(dev).train()
lat, x, p, t = bench.synthetic(1234, dev)
ts = TrainStep(model, lr=8e-4, weight_decay=1e-5, use_graph=False)
ts.bind(p, t, latent_tokens_coord=lat, xcoord=x)
ts.step()
torch.cuda.synchronize()
for k in tables:
    setattr(lib, k, real[k])

g = torch.Generator(device=dev).manual_seed(1)
rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
keep, stream = [], C.c_void_p(torch.cuda.current_stream().cuda_stream)

a_items = tables["gaot_absmax_grouped"]          # (x, ld, rows, cols, out)
words = torch.zeros(len(a_items) * ops.AMAX_SLOTS, device=dev)
a_arr = (L.AbsmaxItem * len(a_items))()
a_src = []
for i, (_, ld, rows, cols, _) in enumerate(a_items):
    m = rnd(rows, ld)
    a_src.append(m)
    a_arr[i] = L.AbsmaxItem(m.data_ptr(), ld, rows, cols, words[i * ops.AMAX_SLOTS:].data_ptr())
print("absmax items:", dict(collections.Counter((r, c, ld) for _, ld, r, c, _ in a_items)), flush=True)

p_items = tables["gaot_split_f16_planes_grouped"]          # (src, ld, rows, cols, absmax, planes_k, planes_t)
p_arr = (L.F16PlanesItem * max(1, len(p_items)))()
for i, (_, ld, rows, cols, _, pk, pt) in enumerate(p_items):
    m = rnd(rows, ld)
    w = torch.zeros(ops.AMAX_SLOTS, device=dev)
    w[0] = float(m.abs().max())
    bufs = [torch.empty(2 * rows * cols, device=dev, dtype=torch.int16) if q else None for q in (pk, pt)]
    keep += [m, w] + bufs
    p_arr[i] = L.F16PlanesItem(m.data_ptr(), ld, rows, cols, w.data_ptr(), *[None if b is None else b.data_ptr() for b in bufs])
print("plane items:", dict(collections.Counter((r, c, ld, bool(pt)) for _, ld, r, c, _, _, pt in p_items)), flush=True)

c_items = tables["gaot_colsum_grouped"]          # (x, ld, out, M, N, out_cols, out_ld)
c_arr = (L.ColsumItem * max(1, len(c_items)))()
for i, (_, ld, _, M, N, oc, old_) in enumerate(c_items):
    m = rnd(M, ld)
    o = torch.zeros((N // oc) * old_ if oc else N, device=dev)
    keep += [m, o]
    c_arr[i] = L.ColsumItem(m.data_ptr(), ld, o.data_ptr(), M, N, oc, old_)
print("colsum items:", dict(collections.Counter((M, N, ld) for _, ld, _, M, N, _, _ in c_items)), flush=True)

calls = [("absmax", lambda: lib.gaot_absmax_grouped(a_arr, len(a_items), stream))]
if p_items:
    calls.append(("planes", lambda: lib.gaot_split_f16_planes_grouped(p_arr, len(p_items), stream)))
if c_items:
    calls.append(("colsum", lambda: lib.gaot_colsum_grouped(c_arr, len(c_items), stream)))
res = collections.defaultdict(list)
for rnd_ in range(3):
    for v in values:
        old = lib.gaot_debug_set_grouped_helpers(v)
        for name, fn in calls:
            for _ in range(5):
                L.check(fn(), name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[(name, v)].append(e0.elapsed_time(e1) / reps * 1e3)
        lib.gaot_debug_set_grouped_helpers(old)
for (name, v), r in sorted(res.items()):
    print(f"{name} grouped_helpers({v}): " + "  ".join(f"{u:.2f}" for u in r) + " us per launch (back to back, device events)", flush=True)
