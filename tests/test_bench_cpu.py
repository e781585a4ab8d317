"""bench.py without a GPU: the --dump-outputs helpers and the command line."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets GPU_MAX_HW_QUEUES at import; keep that out of the rest of the session
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "8"))
    spec = importlib.util.spec_from_file_location("yv_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result_dict(B=3, K=5, cap=6):
    g = torch.Generator().manual_seed(0)
    i32 = lambda *s: torch.randint(1, 9, s, generator=g, dtype=torch.int32)
    f32 = lambda *s: torch.rand(s, generator=g) + 0.5
    return {"num_dets": torch.tensor([[2], [0], [K]], dtype=torch.int32), "bboxes": f32(B, K, 4), "scores": f32(B, K),
            "labels": i32(B, K), "det_count": torch.tensor([1, 0, 3], dtype=torch.int32), "det_box": i32(B, K, 4),
            "det_score": f32(B, K), "det_label": i32(B, K), "crop_rect": i32(B, K, 4), "crop_ok": i32(B, K),
            "crop_list": i32(cap, 6), "crop_total": torch.tensor([4], dtype=torch.int32),
            "crop_part_counts": torch.tensor([3, 1], dtype=torch.int32), "cls_logits": f32(cap, 5), "cls_label": i32(cap),
            "capacity": cap, "done": object()}


def test_infer_outputs_zero_entries_past_the_counts(bench):
    out = _result_dict()
    o = bench.infer_outputs(out)
    assert set(o) == {k for k, v in out.items() if torch.is_tensor(v)}
    for k, n in (("bboxes", [2, 0, 5]), ("scores", [2, 0, 5]), ("labels", [2, 0, 5]), ("det_box", [1, 0, 3]),
                 ("det_score", [1, 0, 3]), ("det_label", [1, 0, 3]), ("crop_rect", [1, 0, 3]), ("crop_ok", [1, 0, 3])):
        for b, m in enumerate(n):
            assert torch.equal(o[k][b, :m], out[k][b, :m]), k
            assert not o[k][b, m:].any(), k
    for k in ("crop_list", "cls_logits", "cls_label"):
        assert torch.equal(o[k][:4], out[k][:4]) and not o[k][4:].any(), k
    for k in ("num_dets", "det_count", "crop_total", "crop_part_counts"):
        assert torch.equal(o[k], out[k]), k


def test_dump_outputs_dtypes_and_limit(bench, tmp_path, monkeypatch):
    x = torch.randn(7, 3).to(torch.bfloat16)
    n = torch.tensor([-3, 0, 2 ** 31 - 1], dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"x": x, "n": n})
    a, b = np.load(tmp_path / "d" / "x.npy"), np.load(tmp_path / "d" / "n.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.float().numpy())
    assert b.dtype == np.float64 and b.tolist() == [-3.0, 0.0, 2147483647.0]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "e"), {"x": torch.zeros(17)})
    assert not (tmp_path / "e").exists()


def test_sample_rows_is_fixed(bench):
    t = torch.arange(50000.0).view(-1, 2)
    s = bench._sample_rows(t, 4096, seed=4321)
    assert s.shape == (4096, 2) and torch.equal(s, bench._sample_rows(t, 4096, seed=4321))
    assert bool((s[1:, 0] > s[:-1, 0]).all())
    assert torch.equal(bench._sample_rows(t[:10], 4096, seed=4321), t[:10])


def test_bench_command_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr
