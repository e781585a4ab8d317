"""Launch-trace recorder of VitTrainer (a helper module, like mx_train_emulation.py; test_trainer_trace_cpu.py is its test).

`record_case` runs two `VitTrainer.step` calls on the CPU with nothing launched and returns, in order, everything the trainer would
have put on a stream:
  * every native wrapper that yvhip.training imports (each function of the yvhip package among the module's globals, bar the host-only
    ones) is replaced by a stub that appends [name, current stream, positional arguments, keyword arguments]: the arguments as the
    wrapper receives them, however the call spells them - the parameters without a default in the signature's order, the others by
    name where the value is not the default;
  * torch.cuda.current_stream / Stream / Event / stream are small fakes that number streams (0 = the main stream) and events in
    creation order and append record / wait_event / wait_stream / enter / exit to the same list;
  * a TorchDispatchMode appends every mutating aten op (copy_, zero_, ...) and every clone / _to_copy: they are kernels too;
  * BucketReducer.reset / ready / finish are appended as well (and run: they are host-only in a one-process run).
Every patch goes through a pytest MonkeyPatch that is undone before `record_case` returns.

Tensor operands are written by name, so that the trace is the same in every process.  Before the first step the trainer's allocations
(P, G, Mo, P16, P16T, w_head_pad, b_head_pad, wmx and _buffers(R), through dicts, lists and tuples) are walked and each storage is
given the first path that reaches it; a case's "allocs" table holds each path's shape, stride and dtype.  An operand is then
    "path"                                   the allocation itself
    "path@offset[shape]/[stride]:dtype"      a view of it: storage offset (if not 0), shape, stride (if not contiguous), dtype (if not
                                             the allocation's)
    ["tmp", shape, stride, dtype]            a tensor whose storage the trainer does not own
Streams are ["stream", id], events ["event", id]; numbers, flags, strings and None stand for themselves.

The fixture tests/golden/vit_trainer_trace.json is written by `python tests/trainer_trace.py --write`, one line per call."""
from __future__ import annotations

import inspect
import json
import os
import sys

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "vit_trainer_trace.json")
HOST_ONLY = ("r128", "require_gpu")                      # functions of the package that launch nothing
R, STEPS, LR, NUM_CLASSES = 3, 2, 0.01, 5
MODELS = {"vit_tiny3_test": (16, 128, 3, 2), "vit_tiny3p8_test": (8, 128, 3, 2)}       # three blocks: block 0 waits on block 2's set
CASES = {
    "bf16": ("vit_tiny3_test", dict(dtype="bf16", cls_tail=False)),
    "bf16_cls_tail": ("vit_tiny3_test", dict(dtype="bf16", cls_tail=True)),
    "mxfp8": ("vit_tiny3_test", dict(dtype="mxfp8", cls_tail=False)),
    "mxfp8_cls_tail": ("vit_tiny3_test", dict(dtype="mxfp8", cls_tail=True)),
    "bf16_p8_long": ("vit_tiny3p8_test", dict(dtype="bf16", cls_tail=False, long_attn=True, long_attn_bwd=True)),
    "mxfp8_cls_tail_p8_long": ("vit_tiny3p8_test", dict(dtype="mxfp8", cls_tail=True, long_attn=True, long_attn_bwd=True)),
}


def _dt(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def _contiguous_stride(shape):
    st, n = [], 1
    for d in reversed(shape):
        st.append(n)
        n *= max(d, 1)
    return st[::-1]


class Recorder:
    def __init__(self):
        self.trace, self.recording = [], False
        self.allocs = {}                                  # storage address -> (path, shape, stride, dtype)
        self.n_streams, self.n_events = 1, 0
        self.stack = [_Stream(self, 0)]

    # ---- the list ---------------------------------------------------------------------------------------
    def add(self, name, args=(), kwargs=None):
        if self.recording:
            rec = [name, self.stack[-1].id, [self.value(a) for a in args]]
            if kwargs:
                rec.append({k: self.value(v) for k, v in kwargs.items()})
            self.trace.append(rec)

    def value(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, _Stream):
            return ["stream", v.id]
        if isinstance(v, _Event):
            return ["event", v.id]
        if isinstance(v, (list, tuple)):
            return [self.value(x) for x in v]
        if isinstance(v, (torch.dtype, torch.device, torch.layout, torch.memory_format)):
            return str(v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"trace: operand of type {type(v).__name__}")

    def tensor(self, t):
        shape, stride = list(t.shape), list(t.stride())
        ent = self.allocs.get(t.untyped_storage().data_ptr()) if t.untyped_storage().nbytes() else None
        if ent is None:
            return ["tmp", shape, stride, _dt(t.dtype)]
        path, a_shape, a_stride, a_dtype = ent
        if t.storage_offset() == 0 and (shape, stride, t.dtype) == (a_shape, a_stride, a_dtype):
            return path
        s = path + (f"@{t.storage_offset()}" if t.storage_offset() else "") + json.dumps(shape, separators=(",", ":"))
        if stride != _contiguous_stride(shape):
            s += "/" + json.dumps(stride, separators=(",", ":"))
        return s if t.dtype == a_dtype else s + ":" + _dt(t.dtype)

    # ---- names ------------------------------------------------------------------------------------------
    def walk(self, path, v):
        if isinstance(v, torch.Tensor):
            if v.untyped_storage().nbytes():
                self.allocs.setdefault(v.untyped_storage().data_ptr(), (path, list(v.shape), list(v.stride()), v.dtype))
        elif isinstance(v, dict):
            for k, x in v.items():
                self.walk(f"{path}.{k}" if path else str(k), x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                self.walk(f"{path}.{i}", x)

    def alloc_table(self):
        return {p: [shape, stride, _dt(dt)] for p, shape, stride, dt in self.allocs.values()}


class _Stream:
    def __init__(self, rec, sid=None):
        self.rec = rec
        if sid is None:
            sid, rec.n_streams = rec.n_streams, rec.n_streams + 1
        self.id = sid

    def wait_event(self, ev):
        self.rec.add("stream.wait_event", (self, ev))

    def wait_stream(self, other):
        self.rec.add("stream.wait_stream", (self, other))


class _Event:
    def __init__(self, rec):
        self.rec, self.id = rec, rec.n_events
        rec.n_events += 1

    def record(self, stream=None):
        self.rec.add("event.record", (self, stream if stream is not None else self.rec.stack[-1]))


class _StreamContext:
    def __init__(self, rec, stream):
        self.rec, self.s = rec, stream

    def __enter__(self):
        self.rec.add("stream.enter", (self.s,))
        self.rec.stack.append(self.s)

    def __exit__(self, *exc):
        self.rec.stack.pop()
        self.rec.add("stream.exit", (self.s,))


class _TorchOps(TorchDispatchMode):
    """Mutating aten ops and copies: kernels that torch itself launches between the native ones."""

    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func._schema.is_mutable or func.overloadpacket.__name__ in ("clone", "_to_copy"):
            self.rec.add("aten." + func.overloadpacket.__name__, args, kwargs)
        return func(*args, **(kwargs or {}))


def _differs(value, default) -> bool:
    if isinstance(value, torch.Tensor) or isinstance(default, torch.Tensor):
        return value is not default
    return type(value) is not type(default) or value != default


def native_stub(rec, name, real, result=lambda given: None):
    """Recording stand-in for the native wrapper `real`.  It appends what the wrapper receives, however the call spells it: the
    parameters without a default in the signature's order, the others by name where the value is not the default.  It returns
    result(arguments by name)."""
    sig = inspect.signature(real)

    def call(*a, **k):
        given = sig.bind(*a, **k).arguments
        pos = [given[p.name] for p in sig.parameters.values() if p.default is p.empty]
        kw = {p.name: given[p.name] for p in sig.parameters.values()
              if p.default is not p.empty and p.name in given and _differs(given[p.name], p.default)}
        rec.add(name, pos, kw)
        return result(given)
    return call


def _patch(mp, rec):
    from yvhip import dist, training
    loss = lambda given: (torch.zeros(1, dtype=torch.float32), torch.zeros_like(given["logits"]))

    natives = {n: v for n, v in vars(training).items()
               if inspect.isfunction(v) and v.__module__ == "yvhip" and n not in HOST_ONLY}
    assert {"linear", "linear_ex", "wgrad", "wgrad_mxfp8", "attention_bwd_long", "sgd_step"} <= set(natives), sorted(natives)
    for n, real in natives.items():
        mp.setattr(training, n, native_stub(rec, n, real, loss) if n == "loss_fwd_bwd" else native_stub(rec, n, real))
    mp.setattr(training, "require_gpu", lambda: None)
    mp.setattr(torch.cuda, "current_stream", lambda device=None: rec.stack[-1])
    mp.setattr(torch.cuda, "Stream", lambda *a, **k: _Stream(rec))
    mp.setattr(torch.cuda, "Event", lambda *a, **k: _Event(rec))
    mp.setattr(torch.cuda, "stream", lambda s: _StreamContext(rec, s))
    for meth in ("reset", "ready", "finish"):
        def traced(self, *a, _real=getattr(dist.BucketReducer, meth), _name="reducer." + meth):
            rec.add(_name, a)
            return _real(self, *a)
        mp.setattr(dist.BucketReducer, meth, traced)


def record_case(case: str) -> dict:
    """{"allocs": {path: [shape, stride, dtype]}, "calls": [...]} of STEPS steps of the case's trainer."""
    from yvhip import engines
    from yvhip.training import VitTrainer
    name, kw = CASES[case]
    kw = dict(dict(long_attn=False, long_attn_bwd=False), **kw)
    rec = Recorder()
    with pytest.MonkeyPatch.context() as mp:
        for model, cfg in MODELS.items():
            mp.setitem(engines.VIT_CFGS, model, cfg)
        _patch(mp, rec)
        tr = VitTrainer(engines.init_vit_wrapper_state(name, NUM_CLASSES, seed=2), name, NUM_CLASSES, device="cpu", **kw)
        for attr in ("P", "G", "Mo", "P16", "P16T", "w_head_pad", "b_head_pad", "wmx"):
            rec.walk(attr, getattr(tr, attr))
        rec.walk("", tr._buffers(R))
        g = torch.Generator().manual_seed(3)
        patches = torch.randn(R * tr.tok, 3 * tr.P_ * tr.P_, generator=g).to(torch.bfloat16)
        labels = torch.randint(0, NUM_CLASSES, (R,), generator=g, dtype=torch.int32)
        rec.recording = True
        with _TorchOps(rec):
            for _ in range(STEPS):
                tr.step(patches, labels, LR)
        rec.recording = False
    return json.loads(json.dumps({"allocs": rec.alloc_table(), "calls": rec.trace}))


def dumps(cases: dict) -> str:
    """The fixture's text: one line per allocation and per call."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    out = []
    for case, t in cases.items():
        allocs = ",\n".join(f"{line(p)}:{line(v)}" for p, v in t["allocs"].items())
        calls = ",\n".join(line(c) for c in t["calls"])
        out.append(f'{line(case)}:{{"allocs":{{\n{allocs}\n}},"calls":[\n{calls}\n]}}')
    return "{\n" + ",\n".join(out) + "\n}\n"


def load_fixture() -> dict:
    with open(FIXTURE, encoding="utf-8") as f:
        return json.load(f)


if __name__ == "__main__":
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "yolov8-vit_amd")]
    text = dumps({case: record_case(case) for case in CASES})
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w", encoding="utf-8") as f:
            f.write(text)
        print(f"wrote {FIXTURE}: {len(text)} bytes, {text.count(chr(10))} lines")
    else:
        sys.stdout.write(text)
