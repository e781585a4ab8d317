"""Global-norm gradient clipping without a GPU: the symbols of yv_grad_clip_ws_bytes / yv_grad_clip_record /
yv_sgd_step_rec / yv_optim_step_rec, every argument check (each is decided on the host before any HIP call, so the pointers are host
addresses that are never dereferenced), the workspace size rule, the parsing of clip_grad / YV_YOLO_CLIP_GRAD, the numpy statement of
the record on hand-worked cases, and the trainer's launches: unchanged with clipping off, pinned by tests/golden/yolo_clip_trace.json
with it on (written by `python tests/test_grad_clip_cpu.py --write`)."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":                              # run as a script: the paths tests/conftest.py sets for pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "yolov8-vit_amd")]

import grad_clip_reference as gc
import trainer_trace as tt
import yolo_trainer_trace as ytt
import yvhip as yv

ERR_ARG, ERR_LIMIT = -1, -2
BUF = (C.c_uint8 * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 256        # a 256-byte aligned host address: never dereferenced
NEW = ("yv_grad_clip_ws_bytes", "yv_grad_clip_record", "yv_sgd_step_rec", "yv_optim_step_rec")
WRAPPERS = ("grad_clip_ws_bytes", "grad_clip_record")
FIXTURE = os.path.join(tt.HERE, "golden", "yolo_clip_trace.json")
FLAG = "YV_YOLO_CLIP_GRAD"
f32 = np.float32
# the fixture's cases: (steps, the unclipped case of yolo_trainer_trace with the same constructor arguments)
CASES = {"sgd": (2, "default"), "adamw_ema_serial": (1, "serial_im2col_adamw_ema")}
CLIP_ALLOCS = ("clip_ws", "clip_rec", "clip_skipped")


def clip_call(g=P, n=1000, grad_scale=1.0, max_norm=10.0, ws=P, ws_bytes=None, rec=P, skipped=P):
    """yv_grad_clip_record on dummy pointers; ws_bytes None: one byte less than yv_grad_clip_ws_bytes asks for, so that a call
    which passes every argument check is stopped by the workspace check, before any launch."""
    if ws_bytes is None:
        ws_bytes = yv.grad_clip_ws_bytes(n) - 1
    return yv.lib.yv_grad_clip_record(C.c_void_p(g), n, grad_scale, max_norm, C.c_void_p(ws), ws_bytes, C.c_void_p(rec),
                                      C.c_void_p(skipped), None)


# ------------------------------------------------------------------------------------------------ symbols, sizes
def test_symbols_in_header_library_and_bindings():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "yv_hip.h")).read()
    for name in NEW:
        assert name + "(" in header, name
        assert hasattr(yv.lib, name), name
        assert name in yv._SIGS and name not in yv.MISSING, name
        assert getattr(yv.lib, name).argtypes == yv._SIGS[name][1], name
    for name in WRAPPERS:
        assert callable(getattr(yv, name)), name
    for name in ("sgd_step", "optim_step"):
        assert inspect.signature(getattr(yv, name)).parameters["scale_rec"].default is None, name


def test_workspace_bytes_grow_with_n_up_to_the_cap():
    ns = [1, 3, 4, 255, 257, 4095, 4096, 4097, 8192, 8193, 100000, 1 << 20, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 1 << 23, 11_000_000,
          1 << 26, 1 << 31, (1 << 31) + 5]
    sizes = [yv.grad_clip_ws_bytes(n) for n in ns]
    assert yv.grad_clip_ws_bytes(0) == 0 and sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s % 8 == 0 for s in sizes)                             # f64 partials, one per workgroup
    cap = sizes[-1]
    at_cap = [n for n, s in zip(ns, sizes) if s == cap]
    assert len(at_cap) >= 5 and at_cap == ns[-len(at_cap):]           # constant once the grid is at its cap
    assert sizes[0] < cap


# ------------------------------------------------------------------------------------------------ argument checks
def test_accepts_the_plain_call_up_to_the_workspace_check():
    """The reference point of the rejections below: the same dummy call with too small a workspace is rejected for the workspace,
    i.e. it passed every argument check."""
    assert clip_call() == ERR_LIMIT
    assert clip_call(ws_bytes=0) == ERR_LIMIT
    assert clip_call(skipped=None) == ERR_LIMIT                       # the counter is optional
    assert clip_call(max_norm=float("inf")) == ERR_LIMIT              # measure, never clip
    assert clip_call(grad_scale=-0.5) == ERR_LIMIT and clip_call(grad_scale=0.0) == ERR_LIMIT
    assert clip_call(n=1) == ERR_LIMIT and clip_call(n=(1 << 31) + 5) == ERR_LIMIT


def test_rejects_null_pointers_and_no_elements():
    for kw in (dict(g=None), dict(ws=None), dict(rec=None), dict(n=0)):
        assert clip_call(ws_bytes=1 << 20, **kw) == ERR_ARG, kw


@pytest.mark.parametrize("max_norm", [0.0, -0.0, -1.0, float("-inf"), float("nan")])
def test_rejects_a_max_norm_that_is_not_positive(max_norm):
    assert clip_call(max_norm=max_norm, ws_bytes=1 << 20) == ERR_ARG


@pytest.mark.parametrize("grad_scale", [float("inf"), float("-inf"), float("nan")])
def test_rejects_a_grad_scale_that_is_not_finite(grad_scale):
    assert clip_call(grad_scale=grad_scale, ws_bytes=1 << 20) == ERR_ARG


def test_rejects_misaligned_gradient_and_workspace():
    for kw in (dict(g=P + 4), dict(g=P + 8), dict(ws=P + 8), dict(ws=P + 4)):
        assert clip_call(ws_bytes=1 << 20, **kw) == ERR_ARG, kw


def test_rec_steps_reject_a_null_record_and_what_the_plain_steps_reject():
    p = C.c_void_p(P)
    sgd, opt = yv.lib.yv_sgd_step_rec, yv.lib.yv_optim_step_rec
    #        p  g  m  n  lr    mu   wd    rec first mirror stream
    ok_sgd = [p, p, p, 8, 1e-3, 0.9, 1e-3, p, 0, None, None]
    for i in (0, 1, 2, 7):
        a = list(ok_sgd); a[i] = None
        assert sgd(*a) == ERR_ARG, i
    for i in (0, 1, 2):                                               # p, g, m: 16-byte aligned
        a = list(ok_sgd); a[i] = C.c_void_p(P + 4)
        assert sgd(*a) == ERR_ARG, i
    a = list(ok_sgd); a[3] = 0
    assert sgd(*a) == 0                                               # nothing to do: no launch
    #        kind p  g  m  v  n  lr    b1   b2     eps   wd    rec step mirror stream
    ok_opt = [2, p, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 5e-4, p, 1, None, None]
    for i in (1, 2, 3, 4, 11):
        a = list(ok_opt); a[i] = None
        assert opt(*a) == ERR_ARG, i
    for kind, step in ((0, 1), (3, 1), (2, 0)):
        a = list(ok_opt); a[0], a[12] = kind, step
        assert opt(*a) == ERR_ARG, (kind, step)
    a = list(ok_opt); a[0], a[4] = 1, None                            # Nesterov has no second moment
    a[5] = 0
    assert opt(*a) == 0


def test_wrappers_refuse_a_record_next_to_a_grad_scale():
    """Decided before any device is touched: host tensors are refused first, so the check is shown on the wrapper's helper."""
    rec = torch.zeros(4)
    with pytest.raises(yv.YvError, match="device"):
        yv.sgd_step(torch.zeros(8), torch.zeros(8), torch.zeros(8), 1e-3, scale_rec=rec)
    fake = torch.zeros(4).as_subclass(ytt._DeviceImages)             # a host tensor that says it is on the device
    yv._chk_rec(fake, 1.0)
    with pytest.raises(yv.YvError, match="grad_scale"):
        yv._chk_rec(fake, 0.5)
    with pytest.raises(yv.YvError, match="four"):
        yv._chk_rec(torch.zeros(5).as_subclass(ytt._DeviceImages))
    with pytest.raises(yv.YvError, match="four"):
        yv._chk_rec(torch.zeros(4, dtype=torch.float64).as_subclass(ytt._DeviceImages))


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_parsing(monkeypatch):
    from yvhip.yolo_training import CLIP_GRAD_ENV, YoloTrainer, clip_grad_value
    from utils import trainYolo as ty
    assert CLIP_GRAD_ENV == FLAG
    assert inspect.signature(YoloTrainer.__init__).parameters["clip_grad"].default is None
    assert inspect.signature(ty.train).parameters["clip_grad"].default is None
    monkeypatch.delenv(FLAG, raising=False)
    assert clip_grad_value(None) is None
    for text, want in (("", None), ("0", None), ("10", 10.0), ("inf", float("inf")), (" 2.5 ", 2.5)):
        monkeypatch.setenv(FLAG, text)
        assert clip_grad_value(None) == want, text
    for text in ("-1", "x", "nan", "-inf"):
        monkeypatch.setenv(FLAG, text)
        with pytest.raises(yv.YvError):
            clip_grad_value(None)
    monkeypatch.setenv(FLAG, "10")                                    # an argument wins over the variable
    assert clip_grad_value(3.0) == 3.0 and clip_grad_value(0) is None and clip_grad_value(float("inf")) == float("inf")
    for bad in (-1, float("nan"), "x", True):
        with pytest.raises(yv.YvError):
            clip_grad_value(bad)


@pytest.mark.parametrize("bad", [-1, float("nan"), -0.5])
def test_train_rejects_a_bad_clip_grad_before_touching_a_gpu(bad, tmp_path, monkeypatch):
    import utils.trainYolo as ty
    monkeypatch.setattr(yv, "require_gpu", lambda: pytest.fail("train() asked for the device before it validated clip_grad"))
    with pytest.raises(yv.YvError, match="clip_grad"):
        ty.train(epochs=1, batch=1, data=str(tmp_path / "none.yaml"), clip_grad=bad)


# ------------------------------------------------------------------------------------------------ the numpy statement
def test_numpy_statement_on_hand_worked_records():
    # S = 400: the norm is 20, above max_norm 10 -> c = 10 / 20.000001 (20 + 1e-6 rounds to the f32 next to 20: ulp(20) = 1.9e-6)
    S, N, c, s, skip = gc.record(400.0, 1.0, 10.0)
    den = f32(20.0) + f32(1e-6)
    assert (S, N, skip) == (f32(400.0), f32(20.0), False)
    assert den == np.nextafter(f32(20.0), f32(30.0)) and c == f32(10.0) / den and c < f32(0.5) and s == c
    # S = 4: the norm is 2, below max_norm -> the coefficient is exactly 1 and the scale is grad_scale, whatever it is
    for gs in (1.0, 1.0 / 3.0, 0.125, -0.5):
        S, N, c, s, skip = gc.record(4.0, gs, 10.0)
        assert N == f32(2.0) * abs(f32(gs)) and c == f32(1.0) and s == f32(gs) and not skip
        assert c.tobytes() == f32(1.0).tobytes() and s.tobytes() == f32(gs).tobytes()
    # grad_scale enters the norm: 20 / 4 = 5 is below 10
    assert gc.record(400.0, 0.25, 10.0)[2] == f32(1.0)
    # max_norm = inf: measure, never clip
    S, N, c, s, skip = gc.record(1e30, 1.0, float("inf"))
    assert np.isfinite(N) and c == f32(1.0) and s == f32(1.0) and not skip
    # a zero gradient: 10 / 1e-6 is far above 1
    assert gc.record(0.0, 1.0, 10.0)[1:] == (f32(0.0), f32(1.0), f32(1.0), False)
    # S = inf (the sum overflowed f32) and S = NaN: skip, coefficient and scale are 0
    for bad in (float("inf"), float("nan")):
        S, N, c, s, skip = gc.record(bad, 1.0, 10.0)
        assert skip and not np.isfinite(N) and c == 0 and s == 0
    assert gc.sum_squares_f64(np.array([3.0, -4.0, 12.0], f32)) == 169.0
    assert gc.ulps(f32(1.0), np.nextafter(f32(1.0), f32(2.0))) == 1 and gc.ulps(f32(-1.0), f32(-1.0)) == 0


# ------------------------------------------------------------------------------------------------ the launches
def record(steps=1, env=None, **kw) -> dict:
    """`steps` steps of yolo_trainer_trace's setting (YOLOv8n, nc 5, 64 x 64, batch 2, its batch) with the constructor arguments kw:
    that module's recorder and patches, plus names for the three buffers clipping owns.  env: the value of YV_YOLO_CLIP_GRAD (None: unset)."""
    from yvhip.yolo_training import YoloTrainer, init_yolo_train_state
    rec = tt.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        for var in ytt.FLAGS + (FLAG, "YV_YOLO_GATHER_WGRAD", "YV_YOLO_FUSED_BN_BWD"):
            mp.delenv(var, raising=False)
        if env is not None:
            mp.setenv(FLAG, env)
        ytt._patch(mp, rec)
        tr = YoloTrainer(init_yolo_train_state(ytt.SCALE, ytt.NC, seed=3), scale=ytt.SCALE, nc=ytt.NC, size=ytt.SIZE, batch=ytt.B,
                         device="cpu", **kw)
        g = torch.Generator().manual_seed(21)
        ctr, wh = torch.rand(ytt.B, ytt.GT, 2, generator=g) * (ytt.SIZE - 30) + 15, torch.rand(ytt.B, ytt.GT, 2, generator=g) * 20 + 8
        batch = dict(images=torch.randint(0, 256, (ytt.B, ytt.SIZE, ytt.SIZE, 3), generator=g,
                                          dtype=torch.uint8).as_subclass(ytt._DeviceImages),
                     gt_boxes=torch.cat([ctr - wh / 2, ctr + wh / 2], -1),
                     gt_labels=torch.randint(0, ytt.NC, (ytt.B, ytt.GT), generator=g, dtype=torch.int32),
                     gt_counts=torch.full((ytt.B,), ytt.GT, dtype=torch.int32))
        ytt._names(rec, tr, batch)
        for name in CLIP_ALLOCS:
            if getattr(tr, name) is not None:
                rec.walk(name, getattr(tr, name))
        rec.recording = True
        with tt._TorchOps(rec):
            for _ in range(steps):
                tr.step(batch["images"], batch["gt_boxes"], batch["gt_labels"], batch["gt_counts"])
        rec.recording = False
        clip = tr.clip_grad
    return dict(json.loads(json.dumps({"allocs": rec.alloc_table(), "calls": rec.trace})), clip_grad=clip)


def record_clipped(case: str) -> dict:
    steps, base = CASES[case]
    return record(steps, clip_grad=10.0, **ytt.CASES[base][1])


@pytest.fixture(scope="module")
def clipped():
    return {case: record_clipped(case) for case in CASES}


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            pytest.fail(f"{what}: call {i} differs\n  recorded: {g}\n  expected: {w}")
    assert len(got) == len(want), what


def test_trace_without_clipping_is_the_default_trace():
    """clip_grad=None with the variable unset: the `default` case of yolo_trainer_trace call for call, allocations included; so is
    clip_grad=0, and the variable at "0"."""
    want = ytt.load_fixture()["default"]
    got = record(ytt.CASES["default"][0])
    assert got["clip_grad"] is None and got["allocs"] == want["allocs"]
    _same(got["calls"], want["calls"], "clip_grad=None")
    assert not any(name in got["allocs"] for name in CLIP_ALLOCS)
    again = record(ytt.CASES["default"][0], clip_grad=0)
    assert again["calls"] == got["calls"] and again["allocs"] == got["allocs"]
    env0 = record(1, env="0")
    assert env0["clip_grad"] is None and env0["allocs"] == want["allocs"]
    assert record(1, env="10")["clip_grad"] == 10.0 and record(1, env="10", clip_grad=0)["clip_grad"] is None


def test_trace_with_clipping_equals_the_fixture(clipped):
    with open(FIXTURE, encoding="utf-8") as f:
        want = json.load(f)
    assert list(want) == list(CASES)
    limit = os.path.getsize(os.path.join(tt.HERE, "golden", "golden.json"))
    assert os.path.getsize(FIXTURE) < 1 << 20
    for case in CASES:
        assert len(tt.dumps({case: want[case]})) < limit, case
        assert clipped[case]["clip_grad"] == 10.0
        assert clipped[case]["allocs"] == want[case]["allocs"], case
        _same(clipped[case]["calls"], want[case]["calls"], case)


@pytest.mark.parametrize("case", list(CASES))
def test_the_clipped_trace_differs_only_where_it_must(clipped, case):
    """Against the unclipped fixture of the same constructor arguments: one grad_clip_record per optimiser step on stream 0, after
    reducer.finish and before the first update; scale_rec=clip_rec on all three group updates (and no grad_scale); three added
    allocations; nothing else."""
    steps, base = CASES[case]
    off, on = ytt.load_fixture()[base], clipped[case]
    assert {k: v for k, v in on["allocs"].items() if k not in CLIP_ALLOCS} == off["allocs"]
    assert sorted(set(on["allocs"]) - set(off["allocs"])) == sorted(CLIP_ALLOCS)
    assert on["allocs"]["clip_rec"] == [[4], [1], "float32"] and on["allocs"]["clip_skipped"] == [[1], [1], "int32"]
    n_param = off["allocs"]["G"][0][0]
    assert on["allocs"]["clip_ws"] == [[max(yv.grad_clip_ws_bytes(n_param), 16)], [1], "uint8"]
    updates = ("sgd_step", "optim_step")
    records = [i for i, c in enumerate(on["calls"]) if c[0] == "grad_clip_record"]
    assert len(records) == steps
    for i in records:
        c = on["calls"][i]
        assert c[1] == 0 and c[2] == ["G", 1.0, 10.0, "clip_ws", "clip_rec"] and c[3] == {"skipped": "clip_skipped"}
        before = [x[0] for x in on["calls"][:i]]
        while before[-1] == "reducer.ready":                          # finish() itself marks what is left ready: lines of its own
            before.pop()
        assert before[-1] == "reducer.finish"                         # right behind the all-reduce ...
        assert [x[0] for x in on["calls"][i + 1:i + 4]] == [updates[case != "sgd"]] * 3          # ... and ahead of the three updates
    stripped = [c for c in on["calls"] if c[0] != "grad_clip_record"]
    assert len(stripped) == len(off["calls"])
    n_updates = 0
    for a, b in zip(stripped, off["calls"]):
        if a[0] in updates:
            n_updates += 1
            assert a[3].get("scale_rec") == "clip_rec" and "grad_scale" not in a[3]
            kw = {k: v for k, v in a[3].items() if k != "scale_rec"}
            assert [a[0], a[1], a[2]] + [kw] == [b[0], b[1], b[2]] + [b[3] if len(b) > 3 else {}]
        else:
            assert a == b
    assert n_updates == 3 * steps


if __name__ == "__main__":
    text = tt.dumps({case: {k: v for k, v in record_clipped(case).items() if k != "clip_grad"} for case in CASES})
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {FIXTURE}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
