"""TEST INFRASTRUCTURE ONLY: numpy statement of `yv_mosaic_augment_ex` (csrc/augment.hip) for one output
image: f32 arithmetic, one rounding per operation, in the kernel's order - flips, per-layer homography with the
projective divide, the `!(w > 0)` fill rule, clamp / floor / four taps / bilinear / round-half-up to a whole 8-bit value,
the truncating blend of two layers, then the 8-bit HSV tables once.

tests/test_yolo_augment_ex_cpu.py anchors it to the committed oracle (oracle/yolo_augment.py `apply_record`) on the
affine single-layer records; everything the oracle does not cover (divide, fill rule, flip bit 1, blend) is stated here."""
import numpy as np

FILL = 114.0
f32 = np.float32


def _lookup(tiles, ri, S, i, j):
    """Canvas pixel (i, j) -> (..., 3) f32: the first placement rectangle that contains it decides, 114 elsewhere."""
    out = np.full(i.shape + (3,), FILL, dtype=f32)
    done = np.zeros(i.shape, dtype=bool)
    n = tiles.shape[0]
    for t in range(int(np.clip(ri[0], 0, 4))):
        tid, x1a, y1a, x2a, y2a, x1b, y1b = (int(v) for v in ri[2 + 8 * t:2 + 8 * t + 7])
        inside = (i >= x1a) & (i < x2a) & (j >= y1a) & (j < y2a) & ~done
        sx, sy = i - x1a + x1b, j - y1a + y1b
        ok = inside & (sx >= 0) & (sx < S) & (sy >= 0) & (sy < S) & (0 <= tid < n)
        if ok.any():
            out[ok] = tiles[tid][sy[ok], sx[ok]].astype(f32)
        done |= inside
    return out


def _rhu(v):
    return np.floor((v + f32(0.5)).astype(f32))


def _mad3(a, b, c, xs, ys):
    return (((a * xs).astype(f32) + (b * ys).astype(f32)).astype(f32) + c).astype(f32)


def sample_layer(tiles, h, ri, xs, ys, S):
    """One layer: (S,S,3) f32 of whole values in [0,255]."""
    h = np.asarray(h, dtype=f32)
    with np.errstate(all="ignore"):
        w = _mad3(h[6], h[7], h[8], xs, ys)
        u = (_mad3(h[0], h[1], h[2], xs, ys) / w).astype(f32)
        v = (_mad3(h[3], h[4], h[5], xs, ys) / w).astype(f32)
        lim = f32(8 * S)
        u = np.where(np.isnan(u), -lim, np.clip(u, -lim, lim)).astype(f32)      # fminf(fmaxf(u, -lim), lim)
        v = np.where(np.isnan(v), -lim, np.clip(v, -lim, lim)).astype(f32)
    uf, vf = np.floor(u), np.floor(v)
    fx, fy = (u - uf).astype(f32), (v - vf).astype(f32)
    gx, gy = (f32(1) - fx).astype(f32)[..., None], (f32(1) - fy).astype(f32)[..., None]
    fx, fy = fx[..., None], fy[..., None]
    i0, j0 = uf.astype(np.int64), vf.astype(np.int64)
    t00, t01 = _lookup(tiles, ri, S, i0, j0), _lookup(tiles, ri, S, i0 + 1, j0)
    t10, t11 = _lookup(tiles, ri, S, i0, j0 + 1), _lookup(tiles, ri, S, i0 + 1, j0 + 1)
    top = ((t00 * gx).astype(f32) + (t01 * fx).astype(f32)).astype(f32)
    bot = ((t10 * gx).astype(f32) + (t11 * fx).astype(f32)).astype(f32)
    rgb = np.clip(_rhu(((top * gy).astype(f32) + (bot * fy).astype(f32)).astype(f32)), 0, 255).astype(f32)
    rgb[~(w > 0)] = FILL                                                         # zero, negative or NaN
    return rgb


def blend(c0, c1, mix):
    """floor(m*c0 + (1-m)*c1) with m = fminf(fmaxf(mix, 0), 1) (NaN -> 0), clamped to [0,255]."""
    m = f32(mix)
    m = f32(0) if np.isnan(m) else f32(min(max(m, f32(0)), f32(1)))
    m1 = f32(f32(1) - m)
    return np.clip(np.floor(((m * c0).astype(f32) + (m1 * c1).astype(f32)).astype(f32)), 0, 255).astype(f32)


def hsv_tail(rgb, lut):
    """The HSV tail of both kernels on whole-valued (S,S,3) f32 -> (S,S,3) u8."""
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    vmax, vmin = np.maximum(R, np.maximum(G, B)), np.minimum(R, np.minimum(G, B))
    diff = (vmax - vmin).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(vmax > 0, _rhu(((f32(255) * diff).astype(f32) / vmax).astype(f32)), f32(0)).astype(f32)
        hr = ((f32(60) * (G - B).astype(f32)).astype(f32) / diff).astype(f32)
        hg = (f32(120) + ((f32(60) * (B - R).astype(f32)).astype(f32) / diff).astype(f32)).astype(f32)
        hb = (f32(240) + ((f32(60) * (R - G).astype(f32)).astype(f32) / diff).astype(f32)).astype(f32)
    h = np.where(vmax == R, hr, np.where(vmax == G, hg, hb))
    h = np.where(diff > 0, h, f32(0)).astype(f32)
    h = np.where(h < 0, (h + f32(360)).astype(f32), h).astype(f32)
    h8 = _rhu((h * f32(0.5)).astype(f32)).astype(np.int64)
    h8 = np.where(h8 >= 180, h8 - 180, h8)
    lut = np.asarray(lut)
    H2, S2, V2 = lut[0][h8].astype(f32), lut[1][s.astype(np.int64)].astype(f32), lut[2][vmax.astype(np.int64)].astype(f32)
    hs = (H2 / f32(30)).astype(f32)
    sec = np.floor(hs)
    fr = (hs - sec).astype(f32)
    sn = (S2 / f32(255)).astype(f32)
    pp = (V2 * (f32(1) - sn).astype(f32)).astype(f32)
    qq = (V2 * (f32(1) - (sn * fr).astype(f32)).astype(f32)).astype(f32)
    tt = (V2 * (f32(1) - (sn * (f32(1) - fr).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    si = sec.astype(np.int64) % 6
    r2 = np.choose(si, [V2, qq, pp, pp, tt, V2])
    g2 = np.choose(si, [tt, V2, V2, qq, pp, pp])
    b2 = np.choose(si, [pp, pp, tt, V2, V2, qq])
    return np.stack([np.clip(_rhu(t), 0, 255) for t in (r2, g2, b2)], axis=-1).astype(np.uint8)


def apply_record_ex(tiles, rec_h, rec_i, mix, lut, S):
    """tiles (N,S,S,3) u8, rec_h (layers,9) f32, rec_i (layers,34) i32, mix scalar (ignored with one layer),
    lut (3,256) u8 -> (S,S,3) u8."""
    rec_h, rec_i = np.asarray(rec_h, dtype=f32).reshape(-1, 9), np.asarray(rec_i).reshape(-1, 34)
    layers = rec_h.shape[0]
    assert layers in (1, 2) and rec_i.shape[0] == layers
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    flip = int(rec_i[0, 1])
    xs = (S - 1 - x if flip & 1 else x).astype(f32)
    ys = (S - 1 - y if flip & 2 else y).astype(f32)
    lay = [sample_layer(tiles, rec_h[k], rec_i[k], xs, ys, S) for k in range(layers)]
    rgb = lay[0] if layers == 1 else blend(lay[0], lay[1], mix)
    return hsv_tail(rgb, lut)
