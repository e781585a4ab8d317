"""GPU: VitEngine(dtype="mxfp8", mid_gemm=True) - the mxfp8 classifier on the "linear_mx_mid" route -
against the bf16 engine, and a RequestSession over such a pipeline against the eager pipeline (the pattern of
test_gpu_request.py, whose helpers it uses)."""
import numpy as np
import pytest
import torch

import test_gpu_request as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME, NC, S, R = "vit_tiny_test", 5, 128, 3
A = 64


@pytest.fixture(scope="module")
def yv():
    import yvhip
    yvhip.require_gpu()
    return yvhip


@pytest.fixture(scope="module")
def vits(yv):
    from yvhip import engines
    sd = engines.init_vit_wrapper_state(NAME, NC, seed=4)
    mk = lambda **kw: engines.VitEngine(sd, NAME, NC, device=DEV, **kw)
    return dict(bf16=mk(), mx=mk(dtype="mxfp8", mid_gemm=False), mx_mid=mk(dtype="mxfp8", mid_gemm=True))


def _feats(e, patches, crops):
    cnt = torch.tensor([crops], dtype=torch.int32, device=DEV)
    f = e.backbone(patches, crops, cnt).clone()
    torch.cuda.synchronize()
    return f[:, :1000].cpu()


@pytest.mark.parametrize("crops", [2, 4])
def test_engine_tracks_bf16_and_restores_the_options(yv, vits, crops):
    """The bounds test_vit_engine_mxfp8_tracks_bf16 sets for the mxfp8 engine: rel-L2 <= 0.12, per-crop cosine >= 0.99."""
    from yvhip import engines
    e16, e8, e8m = vits["bf16"], vits["mx"], vits["mx_mid"]
    g = torch.Generator().manual_seed(crops)
    patches = (torch.rand(crops * e16.tok, 3 * e16.P * e16.P, generator=g) * 2 - 1).to(torch.bfloat16).to(DEV)
    assert yv.get_option("linear_mx_mid") == 0 and yv.get_option("linear_mid") == 0
    # the block products at this capacity: LIN_MX_MID under the option the pass sets, LIN_MX without it
    M, D = crops * e8m.N, e8m.D
    assert M <= engines.MX_MID_GEMM_ROWS
    prods = ((3 * D, D, 0, False), (D, D, yv.EPI_RES_F32, False), (4 * D, D, yv.EPI_GELU, True), (D, 4 * D, yv.EPI_RES_F32, False))
    route = lambda n, k, f, q: (yv.linear_mxfp8_q_route(M, n, k, f | yv.EPI_BIAS, m_dev=True) if q else
                                yv.linear_route(M, n, k, f | yv.EPI_BIAS, mx=True, m_dev=True)).kernel
    assert [route(*p) for p in prods] == [yv.LIN_MX] * 4
    yv.set_option("linear_mx_mid", engines.MX_MID_GEMM_ROWS)
    try:
        assert [route(*p) for p in prods] == [yv.LIN_MX_MID] * 4
    finally:
        yv.set_option("linear_mx_mid", 0)
    b = _feats(e16, patches, crops).double()
    base = _feats(e8, patches, crops)
    assert yv.get_option("linear_mx_mid") == 0
    a = _feats(e8m, patches, crops)
    assert yv.get_option("linear_mx_mid") == 0 and yv.get_option("linear_mid") == 0          # both read 0 after the pass
    err = float((a.double() - b).norm() / b.norm())
    cos = torch.nn.functional.cosine_similarity(a.double(), b, dim=1)
    dist = float((a.double() - base.double()).norm() / base.double().norm())
    print(f"{crops} crops: mxfp8 + mid_gemm vs bf16 rel-L2 {err:.4f}, min cosine {float(cos.min()):.5f}; "
          f"vs mxfp8 without mid_gemm rel-L2 {dist:.3e}")
    assert err <= 0.12, err
    assert float(cos.min()) >= 0.99, float(cos.min())
    # an mxfp8 engine without the flag: the bits it gives with the option never touched, whatever ran in between
    assert torch.equal(_feats(e8, patches, crops), base)


def test_the_pass_restores_a_callers_setting(yv, vits):
    e8m = vits["mx_mid"]
    patches = torch.zeros(e8m.tok, 3 * e8m.P * e8m.P, dtype=torch.bfloat16, device=DEV)
    yv.set_option("linear_mx_mid", 77)
    try:
        _feats(e8m, patches, 1)
        assert yv.get_option("linear_mx_mid") == 77
    finally:
        yv.set_option("linear_mx_mid", 0)


class _Candidates:
    """tr._Candidates for a batch of `batch` images: three disjoint boxes per image, the first counts[b] above the thresholds."""

    def __init__(self, yv, batch):
        g = torch.Generator().manual_seed(11)
        ctr, wh = torch.rand(batch, A, 2, generator=g) * S, torch.rand(batch, A, 2, generator=g) * 40 + 8
        boxes = torch.cat([(ctr - wh / 2).clamp(0, S), (ctr + wh / 2).clamp(0, S)], -1)
        boxes[:, :R] = torch.tensor(tr._Candidates.BOXES, dtype=torch.float32)
        self.yv, self.batch, self.boxes = yv, batch, boxes.contiguous().to(DEV)
        self.scores = torch.full((batch, A, NC), 0.01, device=DEV)

    def set(self, counts):
        s = torch.full((self.batch, A, NC), 0.01)
        for b, d in enumerate(counts):
            for k in range(d):
                s[b, k, (b + k) % NC] = 0.9 - 0.1 * k
        self.scores.copy_(s)

    def attach(self, pipe):
        def detect(images):
            pipe.yolo(images)
            return self.yv.efficient_nms(self.boxes, self.scores, pipe.score_threshold, pipe.iou_threshold, pipe.topk)
        pipe.detect = detect
        return pipe


@pytest.mark.parametrize("batch", [1, 2])
def test_session_against_the_eager_pipeline(yv, vits, batch):
    """Records of a RequestSession equal, bit for bit, those of the eager DetectClassifyPipeline(fit_crops=True) on the same
    engines: a replay launches the kernels of the eager stages, gemm_mx_mid_kernel among them."""
    from yvhip import engines
    from yvhip.pipeline import DetectClassifyPipeline
    from yvhip.request import RequestSession
    yolo = engines.YoloEngine(engines.init_yolo_state("n", NC, seed=1, head_gain=4.0), "n", NC, S, DEV)
    vit = vits["mx_mid"]
    cand = _Candidates(yv, batch)
    pipe = cand.attach(DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R))
    eager = cand.attach(DetectClassifyPipeline(yolo, [vit], max_crops_per_image=R, fit_crops=True))
    ses = RequestSession(pipe)
    g = np.random.default_rng(38 + batch)
    sizes = [(120, 128), (128, 100)][:batch]
    for d in (3, 1, 3, 0, 2):
        cand.set((d,) * batch)
        arrs = tr._pictures(g, sizes)
        want = tr._eager(yv, eager, arrs)
        assert int(want["crop_total"][0]) == batch * d
        got = ses.run(arrs)
        tr._same(got, tr._want(want))
        assert len(got["image"]) == batch * d
    assert ses.stats["replays"] > 0 and ses.stats["captures"] > 0
    assert yv.get_option("linear_mx_mid") == 0
