"""The vector epilogue's aux prefetch (gaot_debug_set_gemm_aux_prefetch): the acts that read a saved activation (SWIGLU_BWD, GELU_BWD,
RELU_BWD) issue a band's aux vectors together, ahead of the band's LDS transpose, instead of pass by pass.  Same values, same order:
everything the products write -- both halves of du, the published magnitude word, what lies between the columns of a wider buffer --
must be equal to the last bit with the switch at 0 and at 1, on the all-DMA tiles (64- and 128-row), the staged split tiles and whatever
the dispatcher picks itself for a shape (fp32-MFMA tiles, skinny paths), at ragged tile edges and short k-loops; and right against float64 and the unfused kernels."""
import pytest
import torch

from gaot_amd import _lib as L

MS = (1, 33, 130, 200)
FS = (4, 68, 132, 260,          # N % 4 == 0 only: no weight planes (staged / fp32 tiles, skinny paths)
      144, 272)                 # N % 16 == 0: the weight has fp16 planes -> the all-DMA tiles where the switch asks for them
KS = (32, 96, 256)
SENTINEL = -12345.0
# tile family -> (gaot_debug_set_gemm_ad, gaot_debug_set_gemm_glds): 5 / 7 put every eligible product on the 128- / 64-row fp16-piece tiles
# (these shapes are far too small for the dispatcher to pick them itself), ad 2 / 3 then take the all-DMA form where the weight has planes
TILES = {"ad64": (2, 7), "ad128": (3, 5), "staged64": (0, 7), "staged128": (0, 5), "default": (1, 4)}


def rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


@pytest.fixture
def switches(request):
    """set_tiles(name), set_pf(on): library switches, restored (and the dispatcher's cached answers dropped) when the test ends"""
    from gaot_amd import ops
    lib = L.load()
    old_ad, old_pf, old_glds = lib.gaot_debug_set_gemm_ad(1), lib.gaot_debug_set_gemm_aux_prefetch(1), lib.gaot_debug_set_gemm_glds(4)
    lib.gaot_debug_set_gemm_ad(old_ad)
    lib.gaot_debug_set_gemm_aux_prefetch(old_pf)
    lib.gaot_debug_set_gemm_glds(old_glds)
    assert old_pf == 1, "the prefetch is the default"

    def restore():
        lib.gaot_debug_set_gemm_ad(old_ad)
        lib.gaot_debug_set_gemm_aux_prefetch(old_pf)
        lib.gaot_debug_set_gemm_glds(old_glds)
        ops._PATH_CACHE.clear()
    request.addfinalizer(restore)

    def set_tiles(name):
        ad, glds = TILES[name]
        lib.gaot_debug_set_gemm_ad(ad)
        lib.gaot_debug_set_gemm_glds(glds)
        ops._PATH_CACHE.clear()          # (the dispatcher's dry-run answers are cached per shape)
    return set_tiles, lib.gaot_debug_set_gemm_aux_prefetch


def _wide(M, cols, pad_l, pad_r, src=None):
    """a [M, cols] column block (exactly M rows) of a wider buffer whose other columns hold a sentinel"""
    buf = torch.full((M, pad_l + cols + pad_r), SENTINEL, device="cuda")
    view = buf[:, pad_l:pad_l + cols]
    if src is not None:
        view.copy_(src)
    return buf, view


def _untouched(buf, pad_l, cols):
    return bool((buf[:, :pad_l] == SENTINEL).all()) and bool((buf[:, pad_l + cols:] == SENTINEL).all())


def _swiglu_ref64(dy, w2, u, F):
    dg = dy.double() @ w2.double()
    u1, u3 = u[:, :F].double(), u[:, F:].double()
    sg = torch.sigmoid(u1)
    return torch.cat([dg * u3 * sg * (1 + u1 * (1 - sg)), dg * u1 * sg], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tiles", list(TILES))
def test_swiglu_bwd_prefetch_is_bit_identical_and_right(tiles, K, switches):
    """du = swiglu'(dY w2; u) through ops.gemm(act=SWIGLU_BWD): switch 0 against switch 1 to the last bit (du, the magnitude word, the
    buffer around du), with tight operands and with operands that are column blocks of wider buffers (ld_aux > 2F, ldc > 2F, u with
    exactly M rows); against float64 (rel < 1e-5) and against the unfused kernels, matmul + gaot_swiglu_bwd (rel < 2e-6) -- the bars of
    test_swiglu_ffn_fused_matches_unfused."""
    from gaot_amd import ops
    set_tiles, set_pf = switches
    lib = L.load()
    assert ops.precision() == "f32" and ops._F16_PIECES[0]
    set_tiles(tiles)
    paths = set()
    for M in MS:
        for F in FS:
            g = torch.Generator().manual_seed(1000 * M + 10 * F + K)
            dy = torch.randn(M, K, generator=g).cuda()
            u = torch.randn(M, 2 * F, generator=g).cuda()
            w2 = torch.nn.Parameter((torch.randn(K, F, generator=g) / F ** 0.5).cuda())
            ref64 = _swiglu_ref64(dy, w2.detach(), u, F)
            for wide in (False, True):
                got = {}
                for pf in (0, 1):
                    set_pf(pf)
                    ops.begin_pass()
                    ops.refresh_weight_amax([w2])
                    if wide:
                        ubuf, uv = _wide(M, 2 * F, 4, 4, u)
                        obuf, ov = _wide(M, 2 * F, 8, 4)
                    else:
                        uv, obuf = u, torch.full((M, 2 * F), SENTINEL, device="cuda")
                        ov = obuf
                    with torch.no_grad():
                        ops.gemm(M, F, K, dy, K, 1, w2.detach(), F, 0, ov, ov.stride(0), act=L.ACT_SWIGLU_BWD, aux_in=uv, ld_aux=uv.stride(0))
                    word = ops.gemm.last_c_amax
                    paths.add(lib.gaot_debug_last_gemm_path())
                    torch.cuda.synchronize()
                    if wide:
                        assert _untouched(obuf, 8, 2 * F), (M, F, K, pf)
                        assert torch.equal(uv, u) and _untouched(ubuf, 4, 2 * F)
                    got[pf] = (ov.clone(), None if word is None else word.clone())
                assert torch.equal(got[0][0], got[1][0]), (M, F, K, wide, float((got[0][0] - got[1][0]).abs().max()))
                assert (got[0][1] is None) == (got[1][1] is None)
                if got[0][1] is not None:
                    assert torch.equal(got[0][1], got[1][1]), (M, F, K, wide)
                    # (a word is 32 slots, one float at the head of each 128-byte line; the tensor's magnitude is their maximum)
                    assert float(got[1][1].view(32, 32)[:, 0].max()) == float(got[1][0].abs().max()), (M, F, K, wide)
                du = got[1][0]
                assert not bool((du == SENTINEL).any())
                assert rel(du, ref64) < 1e-5, (M, F, K, wide, rel(du, ref64))
            # the unfused HIP path: the product, then the gate's gradient as its own kernel
            ops.begin_pass()
            ops.refresh_weight_amax([w2])
            with torch.no_grad():
                dg = ops.matmul_nn(dy, w2.detach())
            du0 = torch.empty(M, 2 * F, device="cuda")
            L.check(lib.gaot_swiglu_bwd(u.data_ptr(), dg.data_ptr(), M, F, du0.data_ptr(), None), "gaot_swiglu_bwd")
            torch.cuda.synchronize()
            assert rel(du, du0) < 2e-6, (M, F, K, rel(du, du0))
    if tiles != "default":
        assert 3 in paths          # the forced tile families did run


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["gelu", "relu"])
@pytest.mark.parametrize("tiles", list(TILES))
def test_act_bwd_prefetch_is_bit_identical_and_right(tiles, act, switches):
    """dx = (dY W) * act'(z) through ops.gemm(act=GELU_BWD / RELU_BWD), the one-vector-per-pass branch: switch 0 against switch 1 to the
    last bit, tight and as column blocks of wider buffers, on every tile family; against float64 (rel < 1e-5: the bar of the SwiGLU case -- the same product
    followed by an elementwise factor of order one)."""
    from gaot_amd import ops
    set_tiles, set_pf = switches
    lib = L.load()
    code = L.ACT_GELU_BWD if act == "gelu" else L.ACT_RELU_BWD
    set_tiles(tiles)
    paths = set()
    for M in MS:
        for N in FS:
            for K in KS:
                g = torch.Generator().manual_seed(1000 * M + 10 * N + K + 7)
                dy = torch.randn(M, K, generator=g).cuda()
                z = torch.randn(M, N, generator=g).cuda()
                w = torch.nn.Parameter((torch.randn(K, N, generator=g) / N ** 0.5).cuda())
                zd = z.double()
                if act == "gelu":
                    fac = 0.5 * (1 + torch.erf(zd / 2 ** 0.5)) + zd * torch.exp(-0.5 * zd * zd) / (2 * torch.pi) ** 0.5
                else:
                    fac = (zd > 0).double()
                ref64 = (dy.double() @ w.detach().double()) * fac
                for wide in (False, True):
                    got = {}
                    for pf in (0, 1):
                        set_pf(pf)
                        ops.begin_pass()
                        ops.refresh_weight_amax([w])
                        if wide:
                            zbuf, zv = _wide(M, N, 4, 8, z)
                            obuf, ov = _wide(M, N, 4, 4)
                        else:
                            zv, obuf = z, torch.full((M, N), SENTINEL, device="cuda")
                            ov = obuf
                        with torch.no_grad():
                            ops.gemm(M, N, K, dy, K, 1, w.detach(), N, 0, ov, ov.stride(0), act=code, aux_in=zv, ld_aux=zv.stride(0))
                        word = ops.gemm.last_c_amax
                        paths.add(lib.gaot_debug_last_gemm_path())
                        torch.cuda.synchronize()
                        if wide:
                            assert _untouched(obuf, 4, N), (M, N, K, pf)
                        got[pf] = (ov.clone(), None if word is None else word.clone())
                    assert torch.equal(got[0][0], got[1][0]), (M, N, K, wide)
                    assert (got[0][1] is None) == (got[1][1] is None)
                    if got[0][1] is not None:
                        assert torch.equal(got[0][1], got[1][1]), (M, N, K, wide)
                    assert not bool((got[1][0] == SENTINEL).any())
                    assert rel(got[1][0], ref64) < 1e-5, (M, N, K, wide, rel(got[1][0], ref64))
    if tiles != "default":
        assert 3 in paths


@pytest.mark.gpu
@pytest.mark.parametrize("tiles,planes", [("default", True), ("ad128", True), ("ad64", True), ("staged128", False)])
def test_normed_swiglu_ffn_gradients_do_not_depend_on_the_prefetch(tiles, planes, switches):
    """ops.normed_swiglu_ffn forward + backward at M = 512, K = 256, F = 1 024 (as the dispatcher runs it, and forced onto the all-DMA tiles --
    weights with their fp16 planes -- and onto the staged ones): the five gradients are equal to the last bit between switch 0 and 1."""
    from gaot_amd import ops
    set_tiles, set_pf = switches
    set_tiles(tiles)
    M, K, F = 512, 256, 1024
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, M // 2, K, generator=g)
    wn = 1.0 + 0.1 * torch.randn(K, generator=g)
    w1, w3, w2 = torch.randn(F, K, generator=g) * 0.06, torch.randn(F, K, generator=g) * 0.06, torch.randn(K, F, generator=g) * 0.03
    dy = torch.randn(2, M // 2, K, generator=g).cuda()
    outs = {}
    for pf in (0, 1):
        set_pf(pf)
        xd = x.cuda().requires_grad_(True)
        prm = [torch.nn.Parameter(t.cuda()) for t in (wn, w1, w3, w2)]
        ops.begin_pass()
        if planes:
            ops.adopt_adjacent_storage([prm[1], prm[2]])
            ops.refresh_weight_amax(prm)
        y = ops.normed_swiglu_ffn(xd, prm[0], 1e-6, prm[1], prm[2], prm[3])
        assert y is not None
        y.backward(dy)
        torch.cuda.synchronize()
        outs[pf] = [y.detach()] + [t.grad.clone() for t in [xd] + prm]
    for a, b, name in zip(outs[0], outs[1], ("y", "dx", "dwn", "dw1", "dw3", "dw2")):
        assert torch.equal(a, b), name
