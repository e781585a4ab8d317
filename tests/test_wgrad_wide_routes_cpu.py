"""The route of the 256 x 128 weight-gradient tiles (yv_wgrad_wide / yv_wgrad_wide_route; gemm_tn_wide_kernel) without a GPU:
the rule restated in Python and compared over a grid, the codes of rejected arguments on dummy pointers, the old entry points'
refusal of tile_n = 256, and VitTrainer(wide_wgrad=True): its launch trace is the default trainer's with each wgrad call
replaced by wgrad_wide(..., routed=True) on the same operands, and the flag's precedence."""
import contextlib
import copy
import ctypes as C
import inspect
import types

import pytest
import torch

import trainer_trace as tt
import yvhip as yv

ERR_ARG = -1
WS = yv.STREAM_WS_BYTES
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
TS, NS, KS = (64, 640, 1088, 6336, 25216), (8, 128, 136, 256, 384, 768, 1000, 2304, 3072), (8, 72, 128, 768, 3072)


@contextlib.contextmanager
def options(**kw):
    old = {k: yv.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            yv.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            yv.set_option(k, v)


def wide_slices(tiles, T, N, K, ws_bytes, n_cu=256, split=0):
    """One round of the 2 * n_cu workgroup slots, at least 128 token rows per slice, at most 16, even when more than two; a forced
    count; the workspace."""
    S = min(2 * (n_cu or 256) // tiles, T // 128, 16)
    if S > 2:
        S -= S % 2
    if split > 0:
        S = split
    S = min(S, ws_bytes // (N * K * 4))
    return S if S >= 2 else 1


def wide_rule(T, N, K, ws_bytes, **kw):
    tiles = -(-N // 256) * -(-K // 128)
    S = wide_slices(tiles, T, N, K, ws_bytes, **kw) if ws_bytes else 1
    return yv.WgradRoute(256, 128, tiles, S, tiles * S)


def routed_wide(T, N, K):
    """mode 0: matrix shapes - N >= 256, K >= 128, more than 16 tiles of 128 x 128 - with at least 25,000 (tile, 64 tokens) pairs."""
    tiles = -(-N // 128) * -(-K // 128)
    return N >= 256 and K >= 128 and tiles > 16 and tiles * (T // 64) >= 25000


def test_route_is_the_rule_over_the_grid():
    seen = set()
    for T in TS:
        for N in NS:
            for K in KS:
                for ws in (0, WS):
                    f, r = yv.wgrad_wide_route(T, N, K, ws_bytes=ws), yv.wgrad_wide_route(T, N, K, routed=True, ws_bytes=ws)
                    assert f == wide_rule(T, N, K, ws), (T, N, K, ws, f)
                    assert f.tile_n == 256 and f.tile_k == 128 and f.tiles == -(-N // 256) * -(-K // 128)
                    assert f.workgroups == f.tiles * f.slices and f.slices >= 1
                    assert f.slices == 1 or (ws and f.slices * N * K * 4 <= ws and T // f.slices >= 128)
                    if not ws:
                        assert f.slices == 1 and r.slices == 1
                    old = yv.wgrad_route(T, N, K, 128, ws_bytes=ws)
                    assert r == (f if routed_wide(T, N, K) else old), (T, N, K, ws, r)
                    assert r.workgroups == r.tiles * r.slices
                    seen.add(r.tile_n)
                    for mode in (False, True):
                        assert yv.wgrad_wide_route(T, N, K, routed=mode, ws_bytes=ws, n_cu=0) == \
                            yv.wgrad_wide_route(T, N, K, routed=mode, ws_bytes=ws, n_cu=256)
    assert seen == {128, 256}


def test_slice_rule_thresholds_and_options():
    assert yv.wgrad_wide_route(6336, 2304, 768) == yv.WgradRoute(256, 128, 54, 8, 432)        # qkv of ViT-B/16 at 32 crops
    assert yv.wgrad_wide_route(6336, 2304, 768, n_cu=128) == yv.WgradRoute(256, 128, 54, 4, 216)
    assert yv.wgrad_wide_route(6336, 768, 768).slices == 16 and yv.wgrad_wide_route(6336, 3072, 768).slices == 6 and yv.wgrad_wide_route(12608, 4096, 1024).slices == 4
    assert yv.wgrad_wide_route(256, 256, 128).slices == 2 and yv.wgrad_wide_route(192, 256, 128).slices == 1
    assert yv.wgrad_wide_route(6336, 768, 3072).slices == 6
    assert yv.wgrad_wide_route(6336, 768, 3072, ws_bytes=768 * 3072 * 4 * 2).slices == 2     # S stays within the workspace
    assert yv.wgrad_wide_route(6336, 768, 3072, ws_bytes=768 * 3072 * 4).slices == 1
    for split in (1, 2, 3, 9):
        with options(wgrad_split=split):                       # forced at any tile count: the wide tile is a matrix-shape kernel
            for T, N, K in ((1088, 1032, 648), (1088, 520, 264), (192, 256, 128), (6336, 2304, 768)):
                assert yv.wgrad_wide_route(T, N, K) == wide_rule(T, N, K, WS, split=split)
                assert yv.wgrad_wide_route(T, N, K).slices == split
    with options(wgrad_split_cap=1):                           # the conv regime's cap is not the wide tile's
        assert yv.wgrad_wide_route(1088, 520, 264) == wide_rule(1088, 520, 264, WS)
    with options(wgrad_split_cap=1, wgrad_split=1):
        assert yv.wgrad_wide_route(1088, 520, 264).slices == 1 and yv.wgrad_route(1088, 520, 264, 128).slices == 1
    assert yv.get_option("wgrad_split") == 0 and yv.get_option("wgrad_split_cap") == 128


def test_routed_mode_thresholds():
    """Every measured shape (profiles/wgrad_wide_layers.txt) on the side it measured, and both sides of each clause."""
    t = lambda T, N, K: yv.wgrad_wide_route(T, N, K, routed=True).tile_n
    for N, K in ((2304, 768), (768, 768), (3072, 768), (768, 3072), (1000, 768)):         # ViT-B/16 at 32 crops: all slower wide
        assert t(6336, N, K) == 128
    assert t(12608, 2304, 768) == 128 and t(12608, 3072, 768) == 256 and t(12608, 768, 3072) == 256      # 64 crops
    assert t(25216, 2304, 768) == 256 and t(25216, 3072, 768) == 256 and t(25216, 768, 3072) == 256      # 128 crops
    assert t(25216, 768, 768) == 128 and t(25088, 768, 768) == 128 and t(128, 1000, 768) == 128
    assert t(12608, 3072, 1024) == 256 and t(12608, 4096, 1024) == 256 and t(12608, 1024, 4096) == 256   # ViT-L/16 at 64 crops
    assert t(12608, 1024, 1024) == 128 and t(12544, 1024, 768) == 128 and t(64, 1000, 1024) == 128
    assert t(11136, 3072, 768) == 256 and t(11072, 3072, 768) == 128       # 144 tiles x 174 = 25,056 against 144 x 173 = 24,912
    assert t(1 << 20, 256, 1152) == 256 and t(1 << 20, 256, 1024) == 128   # 18 tiles against 16
    assert t(1 << 20, 248, 3072) == 128 and t(1 << 20, 3072, 120) == 128   # N < 256, K < 128
    assert t(64, 384, 128) == 128 and t(640, 512, 128) == 128              # the compact cls rows, vit_tiny_test


def test_route_rejects_what_the_launch_rejects():
    out = (C.c_int * 5)()
    f = yv.lib.yv_wgrad_wide_route
    assert f(1088, 256, 128, 0, WS, 256, out) == 0 and f(1088, 256, 128, 1, WS, 256, out) == 0
    for bad in ((1088, 256, 128, 2), (1088, 256, 128, -1), (1088, 256, 128, 256), (1000, 256, 128, 1), (1088, 252, 128, 1),
                (1088, 256, 124, 0), (0, 256, 128, 1), (1088, 0, 128, 1), (1088, 256, 0, 0)):
        assert f(*bad, WS, 256, out) == ERR_ARG, bad
    assert f(1088, 256, 128, 1, WS, 256, None) == ERR_ARG
    assert f(1088, 256, 128, 1, WS, -1, out) == ERR_ARG


def _ww(dY=P, ldy=256, X=P, ldx=128, T=1088, N=256, K=128, dW=P, ldw=128, mode=1):
    return yv.lib.yv_wgrad_wide(dY, ldy, X, ldx, T, N, K, dW, ldw, mode, None)


def test_wide_entry_rejects_bad_arguments():
    """No GPU call is made: every case fails validation first."""
    for m in (2, -1, 128, 256):
        assert _ww(mode=m) == ERR_ARG, m
    for m in (0, 1):
        assert _ww(T=1000, mode=m) == ERR_ARG                  # T & 63
        assert _ww(T=0, mode=m) == ERR_ARG
        assert _ww(N=252, mode=m) == ERR_ARG                   # N & 7
        assert _ww(K=124, mode=m) == ERR_ARG                   # K & 7
        assert _ww(dY=P + 8, mode=m) == ERR_ARG                # misaligned bases
        assert _ww(X=P + 2, mode=m) == ERR_ARG
        assert _ww(dW=P + 4, mode=m) == ERR_ARG
        assert _ww(ldy=252, mode=m) == ERR_ARG                 # misaligned strides
        assert _ww(ldx=124, mode=m) == ERR_ARG
        assert _ww(ldw=126, mode=m) == ERR_ARG
        for name in ("dY", "X", "dW"):
            assert _ww(**{name: None}, mode=m) == ERR_ARG, name


def test_old_entries_still_reject_256():
    out = (C.c_int * 5)()
    assert yv.lib.yv_wgrad_route(1088, 256, 128, 256, WS, 256, out) == ERR_ARG
    assert yv.lib.yv_wgrad_tiled(P, 256, P, 128, 1088, 256, 128, P, 128, 256, None) == ERR_ARG
    assert yv.lib.yv_wgrad_conv3_tiled(P, 256, P, 64, 10, 1088, 256, P, 576, 256, None) == ERR_ARG
    with pytest.raises(yv.YvError):
        yv.wgrad_route(1088, 256, 128, 256)


def test_header_declares_the_new_entries():
    names = yv.header_symbols()
    for n in ("yv_wgrad_wide", "yv_wgrad_wide_route"):
        assert n in names and n in yv._SIGS and n not in yv.MISSING
    assert inspect.signature(yv.wgrad_wide).parameters["routed"].default is False
    assert inspect.signature(yv.wgrad_wide_route).parameters["routed"].default is False
    assert inspect.signature(yv.wgrad).parameters.keys() == {"dy", "x", "dw", "T", "tile_n"}


@pytest.mark.parametrize("case", ["bf16", "bf16_cls_tail", "mxfp8_cls_tail"])
def test_trainer_trace_swaps_wgrad_for_routed_wgrad_wide(monkeypatch, case):
    """The trace of VitTrainer(wide_wgrad=True) is the case's own trace with each wgrad call replaced by wgrad_wide on the same
    operands with routed=True; nothing else differs (same allocations, same order, same streams)."""
    monkeypatch.delenv("YV_VIT_WIDE_WGRAD", raising=False)
    model, kw = tt.CASES[case]
    monkeypatch.setitem(tt.CASES, case + "_wide", (model, dict(kw, wide_wgrad=True)))
    base, wide = tt.record_case(case), tt.record_case(case + "_wide")
    assert wide["allocs"] == base["allocs"]
    want, swapped = copy.deepcopy(base["calls"]), 0
    for c in want:
        if c[0] == "wgrad":
            c[0] = "wgrad_wide"
            kwargs = c[3] if len(c) > 3 else {}
            assert "tile_n" not in kwargs
            c[3:] = [dict(kwargs, routed=True)]
            swapped += 1
    assert swapped >= 2 * tt.STEPS and not any(c[0] == "wgrad_wide" for c in base["calls"])
    if case == "bf16":                                         # 3 blocks x 4 linears, the head and the patch embedding, per step
        assert swapped == tt.STEPS * (3 * 4 + 2)
    assert wide["calls"] == want
    assert not any(c[0] == "wgrad" for c in wide["calls"])
    if case != "bf16":
        assert any(c[0] == "wgrad_wide" and "T" in c[3] for c in wide["calls"])       # the compact cls-row form


def test_flag_precedence(monkeypatch):
    """The argument beats the environment; unset means off; only "1" turns it on."""
    from yvhip import engines
    from yvhip.training import VitTrainer
    assert inspect.signature(VitTrainer.__init__).parameters["wide_wgrad"].default is None
    tt._patch(monkeypatch, tt.Recorder())                      # the trainer is built on the CPU: nothing is launched
    sd = engines.init_vit_wrapper_state("vit_tiny_test", 5, seed=2)
    make = lambda **kw: VitTrainer(sd, "vit_tiny_test", 5, device="cpu", **kw)
    monkeypatch.delenv("YV_VIT_WIDE_WGRAD", raising=False)
    assert make().wide_wgrad is False and make(wide_wgrad=True).wide_wgrad is True and make(wide_wgrad=False).wide_wgrad is False
    monkeypatch.setenv("YV_VIT_WIDE_WGRAD", "1")
    assert make().wide_wgrad is True and make(wide_wgrad=False).wide_wgrad is False
    assert make(cls_tail=True, dtype="mxfp8").wide_wgrad is True
    monkeypatch.setenv("YV_VIT_WIDE_WGRAD", "0")
    assert make().wide_wgrad is False and make(wide_wgrad=True).wide_wgrad is True


def test_cfg_train_wide_wgrad_reaches_the_trainer(monkeypatch):
    """utils.trainClass.fit -> module attribute -> _trainer_for -> VitTrainer(wide_wgrad=True), with a stand-in trainer: absent or
    False passes no argument, True passes wide_wgrad=True, a cached trainer of the other setting is replaced."""
    from utils import trainClass as tc
    from yvhip import training
    made = []

    class StubTrainer:
        def __init__(self, sd, name, nc, img, **kw):
            self.kw, self.dtype = kw, kw.get("dtype", "bf16")
            self.cls_tail, self.wide_wgrad = bool(kw.get("cls_tail", False)), bool(kw.get("wide_wgrad", False))
            made.append(self)

    monkeypatch.setattr(training, "VitTrainer", StubTrainer)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.delenv("YV_VIT_TRAIN_CLS_TAIL", raising=False)
    monkeypatch.delenv("YV_VIT_WIDE_WGRAD", raising=False)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)
            self.model = types.SimpleNamespace(arch="vit_tiny_test", img=224)
            self.num_class = 5

    net = Net()
    cfg = lambda **kw: types.SimpleNamespace(epoch=0, lr=0.01, **kw)
    tc.fit(net, None, None, cfg())
    t0 = tc._trainer_for(net, None)
    assert "wide_wgrad" not in t0.kw and net._yv_train_wide_wgrad is False
    tc.fit(net, None, None, cfg(train_wide_wgrad=False))
    assert tc._trainer_for(net, None) is t0
    tc.fit(net, None, None, cfg(train_wide_wgrad=True))
    t1 = tc._trainer_for(net, None)
    assert t1 is not t0 and t1.kw["wide_wgrad"] is True and "cls_tail" not in t1.kw and "dtype" not in t1.kw
    tc.fit(net, None, None, cfg(train_wide_wgrad=True))
    assert tc._trainer_for(net, None) is t1
    tc.fit(net, None, None, cfg(train_wide_wgrad=True, train_cls_tail=True))
    t2 = tc._trainer_for(net, None)
    assert t2 is not t1 and t2.kw == {**t2.kw, "wide_wgrad": True, "cls_tail": True}
    tc.fit(net, None, None, cfg())
    t3 = tc._trainer_for(net, None)
    assert t3 is not t2 and "wide_wgrad" not in t3.kw and len(made) == 4
    monkeypatch.setenv("YV_VIT_WIDE_WGRAD", "1")               # the environment's trainer differs from the cached default one
    t4 = tc._trainer_for(net, None)
    assert t4 is not t3 and "wide_wgrad" not in t4.kw
