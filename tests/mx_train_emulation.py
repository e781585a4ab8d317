"""CPU emulation of the MXFP8 fine-tune recipe (VitTrainer(dtype="mxfp8")) and the synthetic task of its convergence test.

The four block linears of every transformer block run all three GEMMs on dequantised MX operands (the rule of
yv_quant_mxfp8, pinned to mx_reference.py::emulate_quant by test_gpu_fp8.py), each quantised along its reduction axis:
    forward         Y  = q(X) . q(W)^T            X, W quantised along in-features
    data gradient   dX = q(dY) . q(W^T)^T         dY, W^T quantised along out-features
    weight gradient dW = q(dY^T) . q(X^T)^T       dY^T, X^T quantised along tokens (zero-padded to a multiple of 32)
Operands are rounded to bf16 first (the device quantises bf16 tensors); everything else is the fp32 oracle."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from mx_reference import emulate_quant


def mx_deq(x: torch.Tensor) -> torch.Tensor:
    """(rows, K) -> dequantised f32 of the bf16-rounded values, blocks of 32 along K (K zero-padded to a multiple of 32)."""
    rows, K = x.shape
    xb = x.detach().to(torch.bfloat16).float()
    Kp = (K + 31) // 32 * 32
    if Kp != K:
        xb = torch.cat([xb, torch.zeros(rows, Kp - K)], 1)
    return emulate_quant(xb)[2][:, :K].float()


class MxLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return mx_deq(x) @ mx_deq(w).t() + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = mx_deq(dy) @ mx_deq(w.t().contiguous()).t()
        dw = mx_deq(dy.t().contiguous()) @ mx_deq(x.t().contiguous()).t()
        return dx, dw, dy.sum(0)


def mx_linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    shape = x.shape
    return MxLinear.apply(x.reshape(-1, shape[-1]), w, b).reshape(*shape[:-1], w.shape[0])


def vit_forward_mx(sd, x: torch.Tensor, name: str) -> torch.Tensor:
    """oracle.vit.vit_forward with the block linears of the MX recipe (tokens in (crop, token) order, as on the device)."""
    from oracle.vit import vit_cfg
    P, D, L, H = vit_cfg(name)
    d = D // H
    R = x.shape[0]
    t = F.conv2d(x, sd["model.patch_embed.proj.weight"], sd["model.patch_embed.proj.bias"], stride=P)
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat([sd["model.cls_token"].expand(R, -1, -1), t], dim=1) + sd["model.pos_embed"]
    N = t.shape[1]
    for i in range(L):
        p = f"model.blocks.{i}."
        h = F.layer_norm(t, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], eps=1e-6)
        qkv = mx_linear(h, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"])
        qkv = qkv.reshape(R, N, 3, H, d).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = ((q * (d ** -0.5)) @ k.transpose(-2, -1)).softmax(dim=-1)
        o = (att @ v).transpose(1, 2).reshape(R, N, D)
        t = t + mx_linear(o, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        h = F.layer_norm(t, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], eps=1e-6)
        h = F.gelu(mx_linear(h, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"]))
        t = t + mx_linear(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    c = F.layer_norm(t[:, 0], (D,), sd["model.norm.weight"], sd["model.norm.bias"], eps=1e-6)
    return F.linear(c, sd["model.head.weight"], sd["model.head.bias"])


def grads(sd, x: torch.Tensor, labels: torch.Tensor, name: str, mx: bool):
    """(loss, logits, {name: gradient}) of build_loss under fp32 autograd (mx=False) or the emulated MX recipe (mx=True)."""
    from oracle import train as ot, vit as ov
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    feats = vit_forward_mx(p, x, name) if mx else ov.vit_forward(p, x, name)
    logits = ov.wrapper_head(p, feats)
    loss = ot.build_loss(logits, F.one_hot(labels.long(), 5).float())
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in p.items()}


# ---------------------------------------------------------------------------------------------------- synthetic task
TASK_NAME, TASK_R, TASK_STEPS, TASK_LR, TASK_SEED = "vit_tiny_test", 40, 40, 0.005, 11
TASK_ACC, TASK_LOSS_FRAC = 0.9, 0.4          # reached: accuracy on the batch >= TASK_ACC, last loss <= TASK_LOSS_FRAC * first loss


def synthetic_task():
    """Seeded 5-class task: each class is a fixed random +-1 colour per 16 x 16 patch, blended 50 / 50 with per-image
    noise; TASK_R crops, classes balanced.  Returns (x (R,3,224,224) bf16-representable f32, labels (R,) int32)."""
    g = torch.Generator().manual_seed(TASK_SEED)
    proto = (torch.randint(0, 2, (5, 3, 14, 14), generator=g).float() * 2 - 1)
    proto = proto.repeat_interleave(16, 2).repeat_interleave(16, 3)
    labels = torch.arange(TASK_R, dtype=torch.int32) % 5
    noise = torch.rand(TASK_R, 3, 224, 224, generator=g) * 2 - 1
    x = 0.5 * proto[labels.long()] + 0.5 * noise
    return x.to(torch.bfloat16).float(), labels


def task_init():
    from oracle import vit as ov
    return ov.init_wrapper_state(TASK_NAME, seed=TASK_SEED)


def oracle_train_task(steps: int = TASK_STEPS):
    """fp32 oracle run of the task (SGD momentum 0.9, weight decay 1e-3, constant LR): per-step losses and final accuracy."""
    from oracle import train as ot, vit as ov
    x, labels = synthetic_task()
    params = task_init()
    bufs = {k: None for k in params}
    losses = []
    for _ in range(steps):
        loss, _, gr = grads(params, x, labels, TASK_NAME, mx=False)
        losses.append(float(loss))
        for k in params:
            params[k], bufs[k] = ot.sgd_step(params[k], gr[k], bufs[k], TASK_LR)
    with torch.no_grad():
        logits = ov.wrapper_forward(params, x, TASK_NAME)
    acc = float((logits.argmax(1) == labels.long()).float().mean())
    return losses, acc
