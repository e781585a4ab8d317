"""Reference statements for rectangular detector inputs: oracle/yolo.py's make_anchors and decode with the height and the
width of the network input apart.  A helper, not a test; tests/test_rect_cpu.py checks it equal to oracle.yolo.decode at
H = W."""
import torch

REG_MAX = 16
STRIDES = (8, 16, 32)


def n_anchors(H: int, W: int) -> int:
    return sum((H // s) * (W // s) for s in STRIDES)


def make_anchors_hw(H: int, W: int):
    """Cell centres (+0.5), order y*ws+x, scales 8, 16, 32 concatenated.  Returns anchors (A,2) as (x, y) and strides (A,)."""
    pts, st = [], []
    for s in STRIDES:
        h, w = H // s, W // s
        sx = torch.arange(w, dtype=torch.float32) + 0.5
        sy = torch.arange(h, dtype=torch.float32) + 0.5
        yy, xx = torch.meshgrid(sy, sx, indexing="ij")
        pts.append(torch.stack((xx, yy), -1).view(-1, 2))
        st.append(torch.full((h * w,), float(s)))
    return torch.cat(pts), torch.cat(st)


def decode_hw(raw: torch.Tensor, nc: int, H: int, W: int):
    """raw (B, 64+nc, A) f32 -> boxes (B,A,4) xyxy input pixels, scores (B,A,nc)."""
    B, _, A = raw.shape
    anchors, strides = make_anchors_hw(H, W)
    box = raw[:, :4 * REG_MAX].view(B, 4, REG_MAX, A).permute(0, 1, 3, 2)
    dist = box.softmax(-1) @ torch.arange(REG_MAX, dtype=torch.float32)      # (B,4,A)
    a = anchors.t()[None]                                                     # (1,2,A)
    x1y1 = a - dist[:, :2]
    x2y2 = a + dist[:, 2:]
    boxes = torch.cat([x1y1, x2y2], 1) * strides[None, None]
    return boxes.transpose(1, 2).contiguous(), raw[:, 4 * REG_MAX:].sigmoid().transpose(1, 2).contiguous()


def split_raw(raw: torch.Tensor, nc: int, H: int, W: int):
    """raw (B, 64+nc, A) -> per scale the NHWC parts (B,hs,ws,64) and (B,hs,ws,nc), in anchor order."""
    B, box_l, cls_l, a0 = raw.shape[0], [], [], 0
    for s in STRIDES:
        h, w = H // s, W // s
        part = raw[:, :, a0:a0 + h * w].reshape(B, 64 + nc, h, w).permute(0, 2, 3, 1).contiguous()
        box_l.append(part[..., :64].contiguous())
        cls_l.append(part[..., 64:].contiguous())
        a0 += h * w
    return box_l, cls_l
