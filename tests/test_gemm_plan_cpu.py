"""The GEMM path-selection table, enumerated without a GPU (csrc/gemm_plan.h through gaot_debug_gemm_plan / gaot_gemm_path).

tests/golden/gemm_plans.json is the record of the dispatcher as it stood BEFORE the selection became one function: its gemm_run, compiled
for the host with the launch functions replaced by recorders, run over a grid of shapes / layouts / precisions / split-K requests /
epilogues / alignments under 44 settings of the debug switches, and thinned so that every distinct plan a setting produces on the grid
appears under that setting at least once.  tests/golden/gemm_products.json holds the products of the bench configurations (the keys of
ops._PATH_CACHE after a TrainStep and an inference pass of C2 .. C5, with the path recorded on the GPU at that time) and the tile the same
recorders saw for each.  A rule that moves a product to another kernel, tile or slab count fails here, with the product in the message."""
import ctypes as C
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SETTERS = ["gaot_debug_set_gemm_glds", "gaot_debug_set_gemm_ad", "gaot_debug_set_gemm_ad_flush", "gaot_debug_set_gemm_ad_narrow",
           "gaot_debug_set_gemm_planes", "gaot_debug_set_gemm_tile", "gaot_debug_set_gemm_pieces"]
DEFAULTS = [4, 1, 1, 5, 1, 0, 0]
PLAN = ["path", "family", "tile_rows", "tile_cols", "variant", "slabs", "reduce", "publish_after"]


@pytest.fixture(scope="module")
def lib():
    from gaot_amd.build import build
    from gaot_amd import _lib
    build(verbose=False)
    return _lib.load()


class switches:
    """the seven selection switches set together; the previous values come back in __exit__ whatever happens inside"""

    def __init__(self, lib, values):
        self.lib, self.values = lib, values

    def __enter__(self):
        self.old = []
        try:
            for name, v in zip(SETTERS, self.values):
                self.old.append(getattr(self.lib, name)(v))
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for name, v in zip(SETTERS, self.old):
            getattr(self.lib, name)(v)


def _mod4(base, want):
    """the smallest leading dimension >= base that is `want` modulo 4"""
    return base + (want - base) % 4


def grid_desc(M, N, K, ak, bk, pieces, planes, split_k, raw, act, k_split, colsum, align):
    """a row of gemm_plans.json -> descriptor.  Placeholder pointers: the plan looks at them (null? 16-byte aligned?), never through them.
    align: 0 everything aligned, 1 A off by 4 bytes, 2 ldc no multiple of 4, 3 a misaligned row bias"""
    from gaot_amd._lib import GemmDesc
    d = GemmDesc()
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor = M, N, K, ak, bk
    d.A, d.lda = 0x10000 + (4 if align == 1 else 0), (k_split or K) if ak else M
    d.B, d.ldb = 0x20000, K if bk else N
    ncols = 2 * N if act == 5 else N
    d.C, d.ldc = 0x30000, ncols
    if align == 2:
        d.ldc = ncols + (2 if (ncols + 1) % 4 == 0 else 1)
    if align == 3:
        d.rowbias, d.rowbias_period, d.ld_rowbias = 0x50004, 1, N
    d.act = act
    if act == 5:
        d.aux_in, d.ld_aux = 0x90000, 2 * N
    d.split_k = split_k
    if split_k > 1:
        d.workspace = 0x60000
    if colsum:
        d.colsum = 0x70000
    if k_split:
        d.A2, d.lda2, d.k_split = 0x80000, K - k_split if ak else M, k_split
    d.pieces = pieces
    if pieces == 4:
        d.a_absmax, d.b_absmax = 0xA0000, 0xB0000
        if k_split:
            d.a2_absmax = 0xC0000
    if planes:
        d.b_planes, d.ld_bplanes, d.b_plane_stride = 0xD0000, 2 * K, 16
    d.c_absmax = 0xE0000
    d.raw_slabs = raw
    return d


def product_desc(key):
    """a key of ops._PATH_CACHE -> the descriptor ops.gemm hands to gaot_gemm_path for it (fp16 pieces, placeholder magnitude words)"""
    from gaot_amd._lib import GemmDesc
    (M, N, K, ak, bk, act, split_k, no_colsum, no_bias, no_rowbias, no_rowscale, no_aux_in, no_aux_out, no_residual,
     lda4, ldb4, ldc4, ldaux4, ldr4, misalign, mode, a2, raw, planes) = key
    assert mode == 4, "recorded at the default GAOT_GEMM_MODE"
    d = GemmDesc()
    d.M, d.N, d.K, d.a_kmajor, d.b_kmajor, d.act, d.split_k, d.raw_slabs = M, N, K, ak, bk, act, split_k, int(raw)
    ka = a2[0] if a2 else K
    d.A, d.lda = 0x10000 + misalign, _mod4(ka if ak else M, lda4)
    d.B, d.ldb = 0x20000, _mod4(K if bk else N, ldb4)
    ncols = 2 * N if act == 5 else N
    d.C, d.ldc = 0x30000, _mod4(ncols, ldc4)
    d.ld_aux, d.ldr = _mod4(ncols, ldaux4), _mod4(N, ldr4)
    if a2:
        d.A2, d.k_split, d.lda2 = 0x80000 + a2[2], a2[0], _mod4(K - a2[0] if ak else M, a2[1])
        d.a2_absmax = 0xC0000
    if not no_bias:
        d.bias = 0x40000
    if not no_rowbias:
        d.rowbias, d.rowbias_period, d.ld_rowbias = 0x50000, 1, N
    if not no_rowscale:
        d.rowscale = 0x58000
    if not no_aux_in:
        d.aux_in = 0x90000
    if not no_aux_out:
        d.aux_out = 0x98000
    if not no_residual:
        d.residual = 0xF0000
    if not no_colsum:
        d.colsum = 0x70000
    if split_k > 1:
        d.workspace = 0x60000
    d.pieces, d.a_absmax, d.b_absmax = 4, 0xA0000, 0xB0000
    if planes:
        d.b_planes, d.ld_bplanes, d.b_plane_stride = 0xD0000, 2 * K, 16
    return d


def _plan(lib, d):
    out = (C.c_int32 * 8)()
    rc = lib.gaot_debug_gemm_plan(C.byref(d), out)
    assert rc == 0, (rc, lib.gaot_last_error())
    return list(out)


def test_every_plan_of_the_grid_under_every_switch_setting(lib):
    t = json.load(open(os.path.join(GOLDEN, "gemm_plans.json")))
    assert t["columns"][13:] == PLAN and t["switches"] == [s.replace("gaot_debug_set_gemm_", "") for s in SETTERS]
    assert len(t["settings"]) == 44 and t["settings"][0]["set"] == DEFAULTS
    checked = 0
    for setting in t["settings"]:
        with switches(lib, setting["set"]):
            for i in setting["rows"]:
                row = t["rows"][i]
                d = grid_desc(*row[:13])
                got = _plan(lib, d)
                what = dict(zip(t["columns"][:13], row[:13]))
                assert got == row[13:], f"{what} under {dict(zip(t['switches'], setting['set']))}: {dict(zip(PLAN, got))}, recorded {dict(zip(PLAN, row[13:]))}"
                assert lib.gaot_gemm_path(C.byref(d)) == row[13], (what, setting["set"])
                checked += 1
    assert checked >= 6000
    assert [getattr(lib, s)(v) for s, v in zip(SETTERS, DEFAULTS)] == DEFAULTS          # every switch is back where it was


def test_the_model_products_keep_their_path_and_tile(lib):
    t = json.load(open(os.path.join(GOLDEN, "gemm_products.json")))
    assert sorted(t["products"]) == ["C2", "C3", "C4", "C5"]
    with switches(lib, DEFAULTS):
        for cfg, rows in t["products"].items():
            assert len(rows) >= 17
            for key, path, plan in rows:
                d = product_desc(key)
                what = f"{cfg} {dict(zip(t['key'], key))}"
                assert lib.gaot_gemm_path(C.byref(d)) == path, what
                got = _plan(lib, d)
                assert got == plan, f"{what}: {dict(zip(PLAN, got))}, recorded {dict(zip(PLAN, plan))}"
                assert plan[0] == path, what


def test_a_bad_descriptor_has_no_plan_and_the_last_path_stays(lib):
    d = grid_desc(256, 256, 256, 1, 1, 3, 0, 0, 0, 0, 0, 0, 0)
    before = lib.gaot_debug_last_gemm_path()
    assert _plan(lib, d)[0] == lib.gaot_gemm_path(C.byref(d)) and lib.gaot_debug_last_gemm_path() == before
    d.split_k = 4          # without a workspace
    assert lib.gaot_debug_gemm_plan(C.byref(d), (C.c_int32 * 8)()) != 0 and lib.gaot_gemm_path(C.byref(d)) == -1
    assert lib.gaot_debug_gemm_plan(C.byref(d), None) != 0


def test_the_setters_return_what_they_returned(lib):
    """gaot_debug_set_gemm_glds answers in its own argument's terms (0 / 1 without the split tiles, else 4 .. 9: the 256-row variants
    10 / 11 read back as 4 / 5), gaot_debug_set_gemm_pieces answers 0 for anything outside 1 .. 3, a negative gaot_debug_set_gemm_ad_flush asks"""
    with switches(lib, DEFAULTS):
        back = {0: 0, 1: 1, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 4, 11: 5}
        for on, want in back.items():
            lib.gaot_debug_set_gemm_glds(on)
            assert lib.gaot_debug_set_gemm_glds(4) == want, on
        for n, want in ((1, 1), (2, 2), (3, 3), (4, 0), (0, 0), (-1, 0)):
            lib.gaot_debug_set_gemm_pieces(n)
            assert lib.gaot_debug_set_gemm_pieces(0) == want, n
        assert lib.gaot_debug_set_gemm_ad_flush(-1) == 1 and lib.gaot_debug_set_gemm_ad_flush(0) == 1
        assert lib.gaot_debug_set_gemm_ad_flush(-1) == 0 and lib.gaot_debug_set_gemm_ad_flush(1) == 0
        for name, v in (("gaot_debug_set_gemm_ad", 3), ("gaot_debug_set_gemm_ad_narrow", 31), ("gaot_debug_set_gemm_tile", 6), ("gaot_debug_set_gemm_planes", 0)):
            getattr(lib, name)(v)
            assert getattr(lib, name)(v) == v, name
    for K, s, want in ((256, 4, 4), (256, 64, 8), (100, 3, 2), (2048, 0, 1), (1152, 5, 5), (320, 4, 4), (288, 4, 3)):
        assert lib.gaot_gemm_slab_count(K, s) == want, (K, s)
