"""The decision of yv_linear_ln ("linear_ln_mid" / "linear_ln_fill") as yv_linear_ln_route reports it, the
argument checks of the entry through the raw C ABI, and the option's value around an engine pass; no GPU, 256 CUs."""
import contextlib
import ctypes as C

import pytest

import engine_trace
import engine_trace_ln as etl
import trainer_trace as tt
import yvhip as yv

B, GELU, RES, F32, POS = yv.EPI_BIAS, yv.EPI_GELU, yv.EPI_RES_F32, yv.EPI_OUT_F32, yv.EPI_POSEMB
N_CU = 256
MID_FLOOR, MAX_K = 256, 1024
SHIPPED_FILL = 0                                                 # no shape: the fused launch measured slower everywhere
PAIR = yv.LinearLnRoute(0, 0, 0, 0)
# (tokens + 1, width) of ViT-B/16, ViT-B/8 and ViT-L/16 at 224 x 224
MODELS = {"vit_base_patch16_224": (197, 768), "vit_base_patch8_224": (785, 768), "vit_large_patch16_224": (197, 1024)}


@contextlib.contextmanager
def options(**kw):
    want = dict({"linear_variant": 1, "linear_ln_mid": 0, "linear_ln_fill": SHIPPED_FILL}, **kw)
    old = {k: yv.get_option(k) for k in want}
    try:
        for k, v in want.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def rule(M, N, K, flags, n_cu, variant=1, ln_mid=0, fill=SHIPPED_FILL):
    """The rule in Python: fused where the step exists and the shape is one the kernel takes and 128 x 128 tiles are few."""
    tiles128 = -(-M // 128) * -(-N // 128)
    fused = (variant == 1 and ln_mid > 0 and MID_FLOOR < M <= ln_mid and N % 64 == 0 and K % 64 == 0 and K <= MAX_K and
             not flags & ~(B | GELU | F32) and tiles128 * 8 <= fill * n_cu)
    return yv.LinearLnRoute(1, -(-M // 64), N // 64, -(-M // 64) * (N // 64)) if fused else PAIR


def block_shapes():
    for tok, D in MODELS.values():
        for crops in range(1, 33):
            yield crops * tok, 3 * D, D, B                       # norm1 -> qkv
            yield crops * tok, 4 * D, D, B | GELU                # norm2 -> fc1


def test_the_default_is_the_pair():
    assert yv.get_option("linear_ln_mid") == 0 and yv.get_option("linear_ln_fill") == SHIPPED_FILL      # as shipped
    with options():
        for M, N, K, f in block_shapes():
            assert yv.linear_ln_route(M, N, K, f, n_cu=N_CU) == PAIR
    with options(linear_ln_fill=5):                              # the step does not exist whatever the fill rule says
        for M, N, K, f in block_shapes():
            assert yv.linear_ln_route(M, N, K, f, n_cu=N_CU) == PAIR


def test_the_shipped_fill_rule_takes_no_shape():
    """VitEngine(ln_gemm=True) sets "linear_ln_mid"; under the shipped "linear_ln_fill" every block product stays on the pair."""
    import yvhip.engines as engines
    with options(linear_ln_mid=engines.MID_GEMM_ROWS):
        for M, N, K, f in block_shapes():
            assert yv.linear_ln_route(M, N, K, f, n_cu=N_CU) == PAIR


@pytest.mark.parametrize("fill", [5, 8, 1 << 20])
def test_the_route_is_the_rule(fill):
    import yvhip.engines as engines
    ln_mid = engines.MID_GEMM_ROWS
    with options(linear_ln_mid=ln_mid, linear_ln_fill=fill):
        seen = set()
        for M, N, K, f in block_shapes():
            r = yv.linear_ln_route(M, N, K, f, n_cu=N_CU)
            assert r == rule(M, N, K, f, N_CU, ln_mid=ln_mid, fill=fill), (M, N, K, f)
            seen.add(r.fused)
            if r.fused:
                assert (r.tiles_m, r.tiles_n, r.workgroups) == (-(-M // 64), N // 64, -(-M // 64) * (N // 64))
        assert seen == {0, 1}
        # one crop of a /16 model stays on the pair; two crops fuse (both products: 72 and 96 tiles of 128 x 128)
        assert yv.linear_ln_route(197, 2304, 768, B, n_cu=N_CU) == PAIR
        assert yv.linear_ln_route(394, 2304, 768, B, n_cu=N_CU).fused == 1
        assert yv.linear_ln_route(394, 3072, 768, B | GELU, n_cu=N_CU).fused == 1


def test_each_condition_from_both_sides():
    with options(linear_ln_mid=2048, linear_ln_fill=1 << 20):
        fused = lambda M, N, K, f=B, n_cu=N_CU: yv.linear_ln_route(M, N, K, f, n_cu=n_cu).fused
        assert (fused(256, 768, 768), fused(257, 768, 768)) == (0, 1)           # the floor
        assert (fused(2048, 768, 768), fused(2049, 768, 768)) == (1, 0)         # "linear_ln_mid"
        assert (fused(320, 768, 1024), fused(320, 768, 1088)) == (1, 0)         # layernorm_kernel's width bound
        assert (fused(320, 64, 64), fused(320, 96, 64), fused(320, 64, 96), fused(320, 72, 64)) == (1, 0, 0, 0)
        for f, want in ((0, 1), (B, 1), (B | GELU, 1), (B | F32, 1), (B | GELU | F32, 1), (B | RES, 0), (B | POS, 0),
                        (yv.EPI_SAVE_PRE, 0), (yv.EPI_SILU, 0)):
            assert fused(320, 768, 768, f) == want, f
        yv.set_option("linear_variant", 0)
        assert fused(320, 768, 768) == 0                                        # a forced kernel family: never
        yv.set_option("linear_variant", 1)
    with options(linear_ln_mid=4096):                                           # the fill rule: 5/8 of the CUs in 128 x 128 tiles
        for n_cu in (256, 64):
            for M, N in ((788, 2304), (788, 3072), (1576, 768), (3152, 768), (3152, 2304)):
                for fill in (1, 5, 8):
                    yv.set_option("linear_ln_fill", fill)
                    assert yv.linear_ln_route(M, N, 768, B, n_cu=n_cu) == rule(M, N, 768, B, n_cu, ln_mid=4096, fill=fill)
        yv.set_option("linear_ln_fill", 5)
        assert yv.linear_ln_route(788, 2304, 768, B, n_cu=256).fused == 1       # 7 x 18 = 126 tiles <= 160
        assert yv.linear_ln_route(788, 3072, 768, B, n_cu=256).fused == 0       # 7 x 24 = 168


def test_rejected_arguments_through_the_c_abi():
    """Every check of yv_linear_ln happens on the host before any HIP call."""
    lib = yv.lib
    buf = C.create_string_buffer(64)
    p = (C.addressof(buf) + 15) & ~15                            # a 16-byte aligned dummy base: nothing is dereferenced
    good = dict(x=p, ldx=768, gamma=p, beta=p, eps=1e-6, h=p, ldh=768, w=p, bias=p, out=p, ldo=2304, M=320, N=2304, K=768,
                flags=B, m_dev=None, m_mul=1, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.yv_linear_ln(a["x"], a["ldx"], a["gamma"], a["beta"], a["eps"], a["h"], a["ldh"], a["w"], a["bias"], a["out"],
                                a["ldo"], a["M"], a["N"], a["K"], a["flags"], a["m_dev"], a["m_mul"], a["stream"])
    ARG, LIMIT = -1, -2
    assert call(M=0) == 0                                        # an empty call: accepted, nothing launched
    for name in ("x", "gamma", "beta", "h", "w", "out"):
        assert call(**{name: None}) == ARG, name
        assert call(**{name: p + 4}) == ARG, name                # alignment
    assert call(bias=None) == ARG and call(bias=None, flags=0, M=0) == 0
    assert call(bias=p + 4) == ARG
    assert call(M=-1) == ARG and call(N=0) == ARG and call(K=0) == ARG
    assert call(K=800, ldx=800, ldh=800) == ARG and call(N=2320, ldo=2320) == ARG        # K % 64, N % 64
    assert call(ldx=770) == ARG and call(ldx=704) == ARG         # alignment of the rows of x; a stride below the row
    assert call(ldh=772) == ARG and call(ldh=704) == ARG
    assert call(ldo=2306) == ARG and call(ldo=2240) == ARG
    for f in (B | RES, B | POS, yv.EPI_SILU, yv.EPI_RES_BF16, yv.EPI_SAVE_PRE, yv.EPI_GELU_BWD):
        assert call(flags=f) == ARG, f
    assert call(K=1088, ldx=1088, ldh=1088) == LIMIT
    assert call(K=1024, ldx=1024, ldh=1024, M=0) == 0
    out = (C.c_int * 4)()
    assert lib.yv_linear_ln_route(320, 2304, 768, B, N_CU, None) == ARG
    for M, N, K, n_cu in ((0, 2304, 768, N_CU), (320, 0, 768, N_CU), (320, 2304, 0, N_CU), (320, 2304, 768, -1)):
        assert lib.yv_linear_ln_route(M, N, K, B, n_cu, out) == ARG


def test_the_option_is_restored_after_an_engine_pass():
    """VitEngine(ln_gemm=True) sets "linear_ln_mid" to MID_GEMM_ROWS around its pass and puts the caller's value back - also
    when the pass raises.  The native wrappers are the trace harness's stubs; set_option / get_option are the library's."""
    import yvhip.engines as engines
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        engine_trace._patch(mp, rec)
        seen = []
        mp.setattr(engines, "set_option", yv.set_option)
        mp.setattr(engines, "get_option", yv.get_option)
        mp.setattr(engines, "linear_ln", lambda *a, **k: seen.append(yv.get_option("linear_ln_mid")))
        eng = etl.build(mp, engine_trace.P16, dict(ln_gemm=True, mid_gemm=True), {})
        patches = eng.patch_buffer(engine_trace.CAP)
        for before in (0, 777):
            with options(linear_ln_mid=before):
                mid = yv.get_option("linear_mid")
                eng.backbone(patches, engine_trace.CAP)
                assert yv.get_option("linear_ln_mid") == before and yv.get_option("linear_mid") == mid
        assert seen and set(seen) == {engines.MID_GEMM_ROWS}

        def boom(*a, **k):
            raise RuntimeError("boom")
        mp.setattr(engines, "linear_ln", boom)
        with options(linear_ln_mid=5):
            with pytest.raises(RuntimeError, match="boom"):
                eng.backbone(patches, engine_trace.CAP)
            assert yv.get_option("linear_ln_mid") == 5
