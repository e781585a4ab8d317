"""Reference statements of yv_grad_clip_record (a helper module with no test in it; test_grad_clip_cpu.py and test_gpu_grad_clip.py
use it): the record's last three floats from its first, one rounded numpy-f32 operation per line, and the sum of squares in fp64."""
import numpy as np

f32 = np.float32


def sum_squares_f64(g) -> float:
    """sum_i g[i]^2 in fp64 (each square of an f32 is exact there; numpy adds pairwise: error far below n * 2^-53 relative)."""
    x = np.asarray(g, dtype=np.float64).reshape(-1)
    return float(np.sum(x * x))


def record(S, grad_scale, max_norm):
    """(rec[0], rec[1], rec[2], rec[3], skip) from rec[0] = S: the operations of include/yv_hip.h in their order."""
    with np.errstate(all="ignore"):
        S, gs, mx = f32(S), f32(grad_scale), f32(max_norm)
        root = np.sqrt(S)                          # fsqrt_rn
        N = root * np.abs(gs)                      # fmul_rn
        if not np.isfinite(N):
            return S, N, f32(0.0), f32(0.0), True
        den = N + f32(1e-6)                        # fadd_rn
        q = mx / den                               # fdiv_rn
        c = np.minimum(f32(1.0), q)                # fminf
        s = gs * c                                 # fmul_rn
    assert all(v.dtype == np.float32 for v in (root, N, den, q, c, s))
    return S, N, c, s, False


def ulps(a, b) -> int:
    """Distance of two finite f32 values in units in the last place."""
    key = lambda v: (lambda i: i if i >= 0 else -(i & 0x7fffffff))(int(np.array(v, dtype=np.float32).view(np.int32)))
    return abs(key(a) - key(b))
