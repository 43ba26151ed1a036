"""-m gpu: the small launches of the step in their present form against the form before it, reached through their debug switches: the
same bits, eagerly (twice in a row) and under hipGraph replay (three times: a ticket that did not return to zero would show).
  * the grouped helpers (gaot_absmax_grouped, gaot_split_f16_planes_grouped, gaot_colsum_grouped; gaot_debug_set_grouped_helpers), 70 items
    per call: the plane and column-sum tables hold 64, so the call is cut into two launches;
  * gaot_proj_fold_bwd (gaot_debug_set_proj_fold_split), also against float64;
  * the decoder projection's backward with the row-bias gradient inside the edge-gradient launch (gaot_debug_set_proj_bwd_rowbias)."""
import ctypes as C
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

WORD = 32 * 32                # floats per magnitude word (GAOT_AMAX_SLOTS * GAOT_AMAX_STRIDE)
SHAPES = [(16, 32), (48, 80), (272, 1040)]


def dev():
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def C_void(t):
    return C.c_void_p(t.data_ptr())


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _matrices(n, seed, extra=()):
    """n matrices over SHAPES in turn (then `extra` shapes); every fifth one is a strided view: a column block of a wider matrix.
    Magnitudes differ from item to item (a word that went to the wrong item would show)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (r, c) in enumerate([SHAPES[i % 3] for i in range(n)] + list(extra)):
        scale = 2.0 ** ((i * 7) % 23 - 11)
        if i % 5 == 4:
            wide = (torch.randn(r, c + 48, generator=g) * scale).to(dev())
            out.append(wide[:, 16:16 + c])
        else:
            out.append((torch.randn(r, c, generator=g) * scale).to(dev()))
    return out


def _both_forms(bit, run, outputs, switch="gaot_debug_set_grouped_helpers", on=7):
    """run() with the switch bit cleared (the earlier kernel), then set: eagerly twice, then captured and replayed three times; the outputs
    (cloned after each run, zeroed before each) must be the same bits throughout.  Returns the earlier form's outputs."""
    from gaot_amd import _lib
    set_switch = getattr(_lib.load(), switch)

    def fresh():
        for o in outputs:
            o.zero_()

    def snap():
        torch.cuda.synchronize()
        return [o.clone() for o in outputs]

    def same(got, want, what):
        for n, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (what, n, int((a != b).sum()), float((a.double() - b.double()).abs().max()))

    old = set_switch(on & ~bit)
    try:
        fresh(); run(); want = snap()
        set_switch(on)
        for _ in range(2):
            fresh(); run(); got = snap()
            same(got, want, "eager")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        for _ in range(3):
            fresh(); graph.replay(); got = snap()
            same(got, want, "replay")
    finally:
        set_switch(old)
    return want


def _absmax_call(mats, words):
    from gaot_amd import _lib as L
    arr = (L.AbsmaxItem * len(mats))()
    for i, (t, w) in enumerate(zip(mats, words)):
        arr[i] = L.AbsmaxItem(t.data_ptr(), _ld(t), t.shape[0], t.shape[1], w.data_ptr())
    L.check(L.load().gaot_absmax_grouped(arr, len(mats), _stream()), "gaot_absmax_grouped")


def _slot_max(words):
    return words.view(-1, 32, 32)[:, :, 0].max(dim=1).values


def test_absmax_grouped_words_equal_torch_amax_in_both_forms():
    """70 matrices (and 130: the absmax table holds 96), the three shapes, strided views, plus what the flat stream has to get right:
    vectors stored as [n, 1] (biases, norm weights), element counts that are no multiple of 4, a start 4, 8 and 12 bytes off a 16-byte
    boundary, one element, one row, a strided view of odd width, a matrix of several workgroups with a ragged end"""
    from gaot_amd import _lib
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(70000, generator=g).to(dev())
    odd = [flat[0:1040].view(1040, 1), flat[1041:1041 + 255].view(255, 1), flat[1302:1302 + 77 * 33].view(77, 33),
           flat[4003:4004].view(1, 1), flat[4007:4007 + 6].view(2, 3), flat[4100:4100 + 1001].view(1, 1001),
           flat[6001:6001 + 60001].view(1, 60001), torch.randn(37, 45, generator=g).to(dev())[:, 3:32],
           torch.randn(300, 1, generator=g).to(dev()) * 1e-30, torch.zeros(48, 80, device=dev())]
    for n in (70, 130):
        mats = _matrices(n - len(odd), 11 + n) + odd
        words = torch.zeros(len(mats) * WORD, device=dev())
        views = [words[i * WORD:(i + 1) * WORD] for i in range(len(mats))]
        want = torch.stack([m.abs().amax() for m in mats])
        for bits in (6, 7):          # the earlier kernel, the present one
            old =_lib.load().gaot_debug_set_grouped_helpers(bits)
            try:
                words.zero_()
                _absmax_call(mats, views)
                assert torch.equal(_slot_max(words), want), bits
                _absmax_call(mats, views)          # publishing again changes nothing
                assert torch.equal(_slot_max(words), want), bits
            finally:
                _lib.load().gaot_debug_set_grouped_helpers(old)
        if n == 70:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                _absmax_call(mats, views)
            for _ in range(3):
                words.zero_(); graph.replay()
                assert torch.equal(_slot_max(words), want)
        # nothing but the slot heads of a word is written
        assert float(words.view(-1, 32, 32)[:, :, 1:].abs().sum()) == 0.0


def test_split_f16_planes_grouped_equals_the_earlier_form():
    """70 matrices of the three shapes (strided views among them), planes as stored and transposed, every third without the transposed
    plane: the planes and the words (slot heads and the two spread floats the kernel publishes) are the bits the earlier kernel wrote"""
    from gaot_amd import _lib as L
    g = torch.Generator().manual_seed(6)
    # (the last two: a start 8 bytes off a 16-byte boundary, a row stride that is no multiple of 4 -- no 16-byte tile loads for these)
    mats = _matrices(68, 5) + [torch.randn(48, 100, generator=g).to(dev())[:, 2:82], torch.randn(16, 45, generator=g).to(dev())[:, 4:36]]
    words = torch.zeros(len(mats) * WORD, device=dev())
    views = [words[i * WORD:(i + 1) * WORD] for i in range(len(mats))]
    _absmax_call(mats, views)
    heads = words.clone()
    pk = [torch.zeros(2 * m.numel(), device=dev(), dtype=torch.int16) for m in mats]
    pt = [torch.zeros(2 * m.numel(), device=dev(), dtype=torch.int16) if i % 3 else None for i, m in enumerate(mats)]
    arr = (L.F16PlanesItem * len(mats))()
    for i, m in enumerate(mats):
        arr[i] = L.F16PlanesItem(m.data_ptr(), _ld(m), m.shape[0], m.shape[1], views[i].data_ptr(), pk[i].data_ptr(),
                                 None if pt[i] is None else pt[i].data_ptr())

    def run():
        words.copy_(heads)          # (the outputs are zeroed before every run: the slot heads the kernel reads come back first)
        L.check(L.load().gaot_split_f16_planes_grouped(arr, len(mats), _stream()), "gaot_split_f16_planes_grouped")

    want = _both_forms(2, run, [words] + pk + [p for p in pt if p is not None])
    assert any(int(p.abs().sum()) > 0 for p in want[1:]) and torch.equal(_slot_max(want[0]), _slot_max(heads))
    # the planes are the scaled weight: h + m = s w to the last bit of an fp32 for the largest elements (spot check of one matrix)
    m, w = mats[2], want[0][2 * WORD:3 * WORD]
    sc = 2.0 ** (13 - torch.floor(torch.log2(w.view(32, 32)[:, 0].max())).item())
    r, c = m.shape
    hm = want[1 + 2].view(torch.float16).view(r, c // 16, 2, 16).permute(2, 0, 1, 3).reshape(2, r, c).double()
    big = m.abs().double() * sc >= 0.25
    assert float((((hm[0] + hm[1]) - m.double() * sc).abs() / (m.abs().double() * sc).clamp_min(1e-300))[big].max()) <= 2.0 ** -23


def test_colsum_grouped_equals_the_earlier_form():
    """70 partial-row matrices of the three shapes (2, 5 and 65 tiles: no, a partial and four whole groups of 16 re-placed tiles plus one
    left over) and tall ones (up to 8 192 rows, the tallest the queue admits; 17, 3, 1 and 2 tiles), strided inputs, column-block
    destinations"""
    from gaot_amd import _lib as L
    mats = _matrices(66, 9, extra=[(1040, 272), (2300, 48), (8192, 16), (961, 20)])
    outs, items = [], []
    for i, m in enumerate(mats):
        M, N = m.shape
        if i % 4 == 1 and N % 16 == 0:          # the sums as an [N / 16, 16] column block of a wider matrix
            wide = torch.zeros(N // 16, 40, device=dev())
            outs.append(wide)
            items.append(L.ColsumItem(m.data_ptr(), _ld(m), wide[:, 12:28].data_ptr(), M, N, 16, 40))
        else:
            o = torch.zeros(N, device=dev())
            outs.append(o)
            items.append(L.ColsumItem(m.data_ptr(), _ld(m), o.data_ptr(), M, N, 0, 0))
    arr = (L.ColsumItem * len(items))(*items)

    def run():
        L.check(L.load().gaot_colsum_grouped(arr, len(items), _stream()), "gaot_colsum_grouped")

    want = _both_forms(4, run, outs)
    # and the sums are right: a chain of at most 32 additions per accumulator, 3 to join four of them, 17 in the LDS tree -- within
    # 52 roundings of 2^-24 of the column's sum of magnitudes, 1e-5 with room to spare
    for i, (m, o) in enumerate(zip(mats, want)):
        ref = m.double().sum(0)
        got = o[:, 12:28].reshape(-1) if o.dim() == 2 else o
        assert float((got.double() - ref).abs().max()) <= 1e-5 * float(m.abs().double().sum(0).max()), i
        if o.dim() == 2:
            assert float(o[:, :12].abs().sum()) == 0.0 and float(o[:, 28:].abs().sum()) == 0.0


# ------------------------------------------------------------------ gaot_proj_fold_bwd
@pytest.mark.parametrize("OC", [1, 4])
@pytest.mark.parametrize("Cout", [8, 256])
@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("Q", [1, 17, 4097])
def test_proj_fold_bwd_split_equals_the_earlier_tail(Q, C, Cout, OC):
    """every gradient output present, and each of them absent in turn: the slices computed ahead of the ticket and the slimmer tail give
    the bits of the earlier tail (the workspace is filled with NaNs before every run: nothing stale is read; the ticket is back at zero
    after every run), and they are the node's gradients to the bar tests/test_ops_gpu.py holds this node to (2e-6 in the L2 norm)"""
    from gaot_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(Q * 7 + C * 3 + Cout + OC)
    hw = (torch.randn(OC, C, generator=g) * 0.3).to(dev())
    wr = (torch.randn(C, Cout + 32, generator=g) * 0.2).to(dev())
    wa = wr[:, :Cout]                                            # a column block, as the model hands it over
    rowb = torch.randn(Q, C, generator=g).to(dev())
    gw, gr = torch.randn(OC, Cout, generator=g).to(dev()), torch.randn(Q, OC, generator=g).to(dev())
    ws = torch.empty(int(lib.gaot_proj_fold_workspace(Q, C, OC)), device=dev())
    ticket = torch.zeros(1, device=dev(), dtype=torch.int32)
    full = dict(drowb=torch.zeros(Q, C, device=dev()), dhw=torch.zeros(OC, C, device=dev()), dhb=torch.zeros(OC, device=dev()),
                dwa=torch.zeros(C, Cout + 8, device=dev())[:, :Cout])
    ref = dict(drowb=gr.double() @ hw.double(), dhw=gr.double().t() @ rowb.double() + gw.double() @ wa.double().t(), dhb=gr.double().sum(0),
               dwa=hw.double().t() @ gw.double())
    ptr = lambda t: None if t is None else C_void(t)
    for absent in (None, "drowb", "dhw", "dhb", "dwa"):
        o = {k: (None if k == absent else v) for k, v in full.items()}

        def run():
            ws.fill_(float("nan"))
            L.check(lib.gaot_proj_fold_bwd(ptr(gw), ptr(gr), ptr(hw), C, ptr(wa), wa.stride(0), ptr(rowb), C, Q, C, Cout, OC, ptr(o["drowb"]),
                                           ptr(o["dhw"]), C, ptr(o["dhb"]), ptr(o["dwa"]), full["dwa"].stride(0), ptr(ws), ptr(ticket), _stream()),
                    "gaot_proj_fold_bwd")

        names = [k for k in full if k != absent]
        bases = [full[k] if k != "dwa" else full[k]._base for k in names]          # (zeroed and compared with the columns beside the block)
        want = _both_forms(1, run, bases + [ticket], switch="gaot_debug_set_proj_fold_split", on=1)
        assert int(want[-1]) == 0 and int(ticket) == 0
        for k, w in zip(names, want):
            got = w[:, :Cout] if k == "dwa" else w
            err = float((got.double() - ref[k]).norm() / max(float(ref[k].norm()), 1e-30))
            assert err < 2e-6, (absent, k, err)
            if k == "dwa":
                assert float(w[:, Cout:].abs().sum()) == 0.0


# ------------------------------------------------------------------ decoder projection backward (ops._GNOProjTransform)
@pytest.mark.parametrize("extras", [True, False])
@pytest.mark.parametrize("edges", [True, False])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("OC", [1, 3])
def test_projection_backward_rowbias_in_the_edge_launch(OC, C, B, edges, extras):
    """37 target rows (every fifth empty), 19 source rows, enough edges for three and more partial rows of d_weff -- or none at all --
    with and without row bias and bias: dk, dF, d_weff, d_rowbias, d_bias with the row-bias gradient computed by workgroups appended to
    the edge-gradient launch are the bits of the separate gaot_batchsum launch; d_rowbias is the sum of dy over the batch, added in
    batch order"""
    from gaot_amd import ops, _lib
    from gaot_amd.plan import GeometryPlan
    Q, n_src = 37, 19
    g = torch.Generator().manual_seed(OC * 100 + C + B)
    deg = torch.randint(1, 8, (Q,), generator=g) if edges else torch.zeros(Q, dtype=torch.long)
    deg[::5] = 0
    splits = torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)])
    E = int(splits[-1])
    assert E == 0 or int(_lib.load().gaot_gno_lift_edge_grad_parts(E, C)) >= 3
    index = torch.randint(0, n_src, (E,), generator=g)
    plan = GeometryPlan(index.to(dev()), splits.to(dev()), n_src)
    k = torch.randn(E, C, generator=g).to(dev()).requires_grad_()
    f = torch.randn(B, n_src, C, generator=g).to(dev()).requires_grad_()
    weff = (torch.randn(OC, C, generator=g) * 0.3).to(dev()).requires_grad_()
    rowb = torch.randn(Q, OC, generator=g).to(dev()).requires_grad_() if extras else None
    bs = torch.randn(OC, generator=g).to(dev()).requires_grad_() if extras else None
    a = torch.rand(max(E, 1), generator=g).to(dev())
    dy = torch.randn(B, Q, OC, generator=g).to(dev())
    params = [k, f, weff] + ([rowb, bs] if extras else [])
    outs = [torch.zeros_like(p) for p in params]

    def run():
        if E > 0:
            y = ops.gno_proj_transform(k, f, weff, rowb, bs, plan, a)
            grads = torch.autograd.grad(y, params, dy)
        else:          # (the forward kernels refuse an empty edge list: the backward node alone, as autograd would call it)
            ctx = NS(saved_tensors=(k.detach(), f.detach(), weff.detach(), a), meta=(True, rowb.shape if extras else None, extras), plan=plan,
                     needs_input_grad=(True, True, True, extras, extras, False, False))
            grads = [gr for gr in ops._GNOProjTransform.backward(ctx, dy)[:5] if gr is not None]
        for o, gr in zip(outs, grads):
            o.copy_(gr)

    want = _both_forms(1, run, outs, switch="gaot_debug_set_proj_bwd_rowbias", on=1)
    if extras:
        ref = torch.zeros(Q, OC, device=dev())
        for b in range(B):
            ref = ref + dy[b]
        assert torch.equal(want[3], ref)
        assert float((want[4].double() - dy.double().sum((0, 1))).abs().max()) <= 1e-5 * float(dy.abs().double().sum((0, 1)).max())
