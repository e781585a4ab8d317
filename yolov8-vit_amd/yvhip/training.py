"""ViT fine-tune step on the HIP path (reference loop utils/trainClass.py:374-420).

One `VitTrainer.step(patches, labels, lr)` = forward (activations kept) -> build_loss (fused kernel) ->
backward -> [data-parallel: bucketed gradient SUM all-reduce over RCCL, overlapped with the rest of
backward] -> SGD(momentum 0.9, weight_decay 1e-3) on fp32 master weights -> bf16 working copies refreshed.

Memory layout (sized for 288 GB of HBM: nothing is recomputed except softmax probabilities):
  * parameters, gradients and momentum are three FLAT fp32 buffers in state-dict order (64-float aligned
    slots): the optimizer is ONE kernel launch and all-reduce buckets are plain slices;
  * the bf16 working weights are ONE flat mirror of the master buffer, written by the SGD kernel itself;
  * dgrad (dY . W) and wgrad (dY^T . X) read their reduction-major operands with the gfx950 transposing LDS
    read, so neither W^T copies nor transposed activations exist; wgrad operands carry 64-row zero padding.
Gradients arrive in exactly the reverse of the flat order (head first, patch-embed last), so a bucket is
complete - and its all-reduce can start - as soon as backward has passed its lowest offset.

dtype="mxfp8" (opt-in): the four block linears (qkv, proj, fc1, fc2) run all three of their GEMMs on
MXFP8 operands (e4m3 + one E8M0 scale per 32 elements of the reduction axis): forward Y = X . W^T and data gradient
dX = dY . W on the block-scaled MFMA with the trainer epilogues (yv_linear_mxfp8_ex), weight gradient dW = dY^T . X from
the token-quantised column forms of both operands (yv_wgrad_mxfp8).  Every bf16 activation / gradient operand is quantised by
ONE pass of yv_quant_mxfp8_2d that writes the row form (for the forward / data-gradient GEMM) and the column form (for the
weight gradient); the weights are re-quantised from the bf16 mirror after every optimizer step (W row-wise and, from the same
read, W^T row-wise).  Patch-embed, heads, attention, LayerNorm, GELU, the residual stream, master weights, gradients, SGD and
the all-reduce keep their bf16 / f32 form; the structure of forward, backward and optimizer step is that of dtype="bf16".

Where the block is written: its op order (LN1, qkv, attention, proj + residual, LN2, fc1 + GELU, fc2 + residual, and the reverse
chain) stands once per direction in _block_forward / _block_backward and once per direction for the cls-row last block in
_tail_forward / _tail_backward.  None of the four tests the recipe: _product, _dgrad and _wgrad pick the bf16 or MX form of a
product, and _side_stream_epilogue is the one copy of the side-stream section (bias column sums, weight gradients, ready buckets,
the "done" event of the parity protocol).  tests/test_trainer_trace_cpu.py pins the launch order.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import (EPI_GELU, EPI_GELU_BWD, EPI_OUT_F32, EPI_POSEMB, EPI_RES_F32, EPI_SAVE_PRE, YvError, attention_bwd,
               attention_bwd_long, attention_bwd_short, attention_cls_bwd, attention_cls_train, attention_long, attention_train, cast_colsum, cls_rows, colsum_bf16, head_bwd, layernorm,
               layernorm_bwd, lib, linear, linear_ex, linear_mxfp8_ex, linear_nn, loss_fwd_bwd, quant_mxfp8_2d, r128, require_gpu, sgd_step,
               token_reduce, transpose_bf16_batched, wgrad, wgrad_mxfp8, wgrad_wide, wrapper_head)
from .engines import _env_flag, vit_cfg


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


BLOCK_LINEARS = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")
# a block's weight gradients in launch order: (weight, gradient operand in the parity set, its MX column form, activation)
BLOCK_WGRADS = (("mlp.fc2.weight", "dxb_fc2", "c_fc2", "g"), ("mlp.fc1.weight", "dwide", "c_wide", "h2"),
                ("attn.proj.weight", "dxb_proj", "c_proj", "o"), ("attn.qkv.weight", "dqkv", "c_qkv", "h1"))


def check_train_dtype(dtype: str, D: int):
    """The recipes VitTrainer accepts: "bf16" (default) and "mxfp8" (D, 3D and 4D - every reduction and output width of the
    block linears - multiples of 128, i.e. D % 128 == 0: ViT-B/16, B/8, L/16 and the vit_tiny*_test models)."""
    if dtype not in ("bf16", "mxfp8"):
        raise YvError(f"VitTrainer dtype must be 'bf16' or 'mxfp8', not {dtype!r}")
    if dtype == "mxfp8" and D % 128:
        raise YvError(f"VitTrainer(dtype='mxfp8') needs an embedding width that is a multiple of 128 (got {D})")


class VitTrainer:
    def __init__(self, state: Dict[str, torch.Tensor], name: str, num_classes: int = 5, img: int = 224,
                 device: str = "cuda:0", momentum: float = 0.9, weight_decay: float = 1e-3,
                 bucket_mb: float = 32.0, dtype: str = "bf16", long_attn: Optional[bool] = None,
                 long_attn_bwd: Optional[bool] = None, cls_tail: Optional[bool] = None, wide_wgrad: Optional[bool] = None,
                 short_attn_bwd: Optional[bool] = None):
        """long_attn (opt-in, both dtypes): the forward attention runs as attention_long(..., lse=...) in place of attention_train
        where the token count exceeds 224 (a shorter-sequence trainer accepts the flag and keeps attention_train); attention_bwd
        is the same and consumes that lse.  None reads the environment variable YV_VIT_LONG_ATTN ("1" = on, unset = off).

        long_attn_bwd (opt-in, both dtypes, independent of long_attn): the attention backward runs as attention_bwd_long in place
        of attention_bwd where the token count exceeds 224 (a shorter-sequence trainer accepts the flag and keeps attention_bwd).
        Same operands, same bits in every gradient.  None reads YV_VIT_LONG_ATTN_BWD ("1" = on, unset = off).

        cls_tail (opt-in, both dtypes, independent of the two flags above): the last block runs on the cls
        rows.  Nothing after it reads tokens 1..N-1, so the gradient that enters it is zero on every other row and stays zero down
        to its attention: LN1 and the qkv product (forward, data gradient, weight gradient) keep every row, the attention is
        attention_cls_train / attention_cls_bwd (one query per crop; dK and dV for every key), and proj, LN2, fc1, GELU and fc2 with
        their gradients run on compact (R, *) operands.  Blocks 0..L-2 are untouched.  With dtype="mxfp8" the cls-row products run
        in bf16 on the bf16 mirror (forward `linear`, data gradients `linear_nn` on the master layout, weight gradients `wgrad`):
        quantising a 32-row operand buys nothing, so the last block's small products are more precise than the MX ones; its
        full-row qkv product and that product's two gradients stay MX.  A model of more than 8192 tokens accepts the flag and runs
        the full block.  None reads YV_VIT_TRAIN_CLS_TAIL ("1" = on, unset = off).

        wide_wgrad (opt-in, both dtypes, independent of the flags above): every bf16 weight gradient - the
        block linears, the compact cls-row form, the head and the patch embedding - is launched as wgrad_wide(..., routed=True) in
        place of wgrad on the same operands: 256 x 128 output tiles where wgrad_wide_route picks them, wgrad's own launch elsewhere.
        The MX column-form launches are not touched.  None reads YV_VIT_WIDE_WGRAD ("1" = on, unset = off).

        short_attn_bwd (opt-in, both dtypes, independent of the flags above): the attention backward runs as
        the one-launch attention_bwd_short in place of attention_bwd where the token count is at most 224 (a longer-sequence
        trainer accepts the flag and is unaffected; with cls_tail the last block keeps attention_cls_bwd).  Same operands, same
        bits in every gradient.  None reads YV_VIT_SHORT_ATTN_BWD ("1" = on, unset = off)."""
        self.long_attn = _env_flag(long_attn, "YV_VIT_LONG_ATTN")
        self.long_attn_bwd = _env_flag(long_attn_bwd, "YV_VIT_LONG_ATTN_BWD")
        self.cls_tail = _env_flag(cls_tail, "YV_VIT_TRAIN_CLS_TAIL")
        self.wide_wgrad = _env_flag(wide_wgrad, "YV_VIT_WIDE_WGRAD")
        self.short_attn_bwd = _env_flag(short_attn_bwd, "YV_VIT_SHORT_ATTN_BWD")
        self.P_, self.D, self.L, self.H = vit_cfg(name)
        check_train_dtype(dtype, self.D)
        require_gpu()
        self.dtype = dtype
        self.name, self.nc, self.img, self.dev = name, num_classes, img, torch.device(device)
        self.tok = (img // self.P_) ** 2
        self.N = self.tok + 1
        self._tail = self.cls_tail and self.N <= 8192          # the cls kernels keep one query's scores in LDS
        self.momentum, self.wd = momentum, weight_decay
        self.steps = 0
        # ---- flat fp32 parameter / gradient / momentum buffers --------------------------------
        self.names: List[str] = list(state.keys())
        self.shapes = {k: tuple(state[k].shape) for k in self.names}
        self.off: Dict[str, int] = {}
        o = 0
        for k in self.names:
            self.off[k] = o
            o += _r64(state[k].numel())
        self.total = o
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=self.dev)
        self.P, self.G, self.Mo = z(o), z(o), z(o)
        for k in self.names:
            self.p(k).copy_(state[k].to(self.dev, torch.float32))
        # ---- bf16 working copies of the GEMM weights: ONE flat bf16 mirror of P (same offsets), refreshed by the
        # SGD kernel itself; a GEMM weight is a view into it, used as (N,K) by forward / wgrad and, through the
        # transposing-read kernel, as the reduction-major operand of dgrad (no W^T copies)
        D = self.D
        self.P16 = torch.zeros(o, dtype=torch.bfloat16, device=self.dev)
        self.gemm_w: Dict[str, tuple] = {}                 # key -> (N, K, wb view (N,K))
        def reg(key, N, K):
            self.gemm_w[key] = (N, K, self._view16(key).reshape(N, K))
        reg("model.patch_embed.proj.weight", D, 3 * self.P_ * self.P_)
        for i in range(self.L):
            b = f"model.blocks.{i}."
            reg(b + "attn.qkv.weight", 3 * D, D); reg(b + "attn.proj.weight", D, D)
            reg(b + "mlp.fc1.weight", 4 * D, D); reg(b + "mlp.fc2.weight", D, 4 * D)
        reg("model.head.weight", 1000, D)
        self.w_head_pad = torch.zeros((1024, D), dtype=torch.bfloat16, device=self.dev)   # dgrad reduces over 1024
        self.b_head_pad = z(1024)
        # ---- TRANSPOSED bf16 mirror of the block linears (same offsets; (K, N) row-major): the data gradient dX = dY . W is then
        # an ordinary linear on W^T and runs on the persistent forward GEMM (round 3; the transposing-read kernel on the master
        # layout ran at 0.12 of the MFMA roof and was a quarter of the step).  Refreshed after every optimizer step by four
        # batched transposes (one per linear of a block, batch = depth): 170 MB read + 170 MB written, ~1 % of a step.
        # (dtype="mxfp8": no reader - the data gradients take W^T from the column form of the weight quantiser - not allocated)
        self.P16T = torch.zeros(o, dtype=torch.bfloat16, device=self.dev) if dtype == "bf16" else None
        self.blk_stride = (self.off["model.blocks.1.attn.qkv.weight"] - self.off["model.blocks.0.attn.qkv.weight"]) if self.L > 1 else 0
        for i in range(1, self.L):
            for w in BLOCK_LINEARS:
                if self.off[f"model.blocks.{i}.{w}"] - self.off[f"model.blocks.0.{w}"] != i * self.blk_stride:
                    raise YvError("state dict: blocks are not laid out with one stride")
        # ---- MXFP8 weight operands (dtype="mxfp8"): per block linear W (N, K) row-wise and W^T (K, N) row-wise, both quantised
        # from the bf16 mirror by one yv_quant_mxfp8_2d pass (its column form of W IS W^T quantised along N)
        self.wmx: Dict[str, tuple] = {}
        if dtype == "mxfp8":
            u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=self.dev)
            for i in range(self.L):
                for w in BLOCK_LINEARS:
                    key = f"model.blocks.{i}.{w}"
                    N_, K_ = self._nk(key)
                    self.wmx[key] = (u8(N_, K_), u8(K_ // 128, r128(N_), 4), u8(K_, N_), u8(N_ // 128, r128(K_), 4))
        self.P16.copy_(self.P)                               # initial cast (plumbing); afterwards the SGD kernel mirrors
        self.refresh_working_copies()
        self._bufs: Dict[int, dict] = {}
        self.s_w = None                                      # side stream of the weight gradients (backward)
        from .dist import BucketReducer
        self.reducer = BucketReducer(self.G, int(bucket_mb * 1024 * 1024 / 4))

    # ---- views ----------------------------------------------------------------------------------
    def _span(self, k) -> slice:
        """Parameter k's elements in a flat buffer."""
        return slice(self.off[k], self.off[k] + math.prod(self.shapes[k]))

    def _view(self, flat, k):
        return flat[self._span(k)].view(self.shapes[k])

    def _view16(self, k):
        return self.P16[self._span(k)]

    def _nk(self, key: str):
        """(N, K) of a GEMM weight."""
        return self.gemm_w[key][:2]

    def _g2d(self, key: str) -> torch.Tensor:
        """The gradient of a GEMM weight as the (N, K) matrix a weight-gradient product writes."""
        return self.g(key).reshape(self._nk(key))

    def p(self, k):
        return self._view(self.P, k)

    def g(self, k):
        return self._view(self.G, k)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {k: self.p(k).detach().clone() for k in self.names}

    def grad_dict(self) -> Dict[str, torch.Tensor]:
        return {k: self.g(k).detach().clone() for k in self.names}

    def refresh_working_copies(self):
        """Only the 1000 -> 1024 padded head copies need touching: everything else is a view of the mirror."""
        self.w_head_pad[:1000].copy_(self.gemm_w["model.head.weight"][2])
        self.b_head_pad[:1000].copy_(self.p("model.head.bias"))
        if self.dtype == "mxfp8":
            # MX operands of the block linears (this recipe has no transposed bf16 mirror)
            for key, (wq, ws, wtq, wts) in self.wmx.items():
                quant_mxfp8_2d(self.gemm_w[key][2], wq, ws, wtq, wts)
            return
        for w in BLOCK_LINEARS:
            key = "model.blocks.0." + w
            N, K = self._nk(key)
            o = self.off[key]
            transpose_bf16_batched(self.P16[o:], self.P16T[o:], N, K, self.L, self.blk_stride, self.blk_stride)

    def wt(self, key: str) -> torch.Tensor:
        """W^T of a block linear, (K, N) row-major bf16 (view of the transposed mirror)."""
        N, K = self._nk(key)
        o = self.off[key]
        return self.P16T[o:o + N * K].view(K, N)

    # ---- buffers ----------------------------------------------------------------------------------
    def _buffers(self, R: int) -> dict:
        if R in self._bufs:
            return self._bufs[R]
        dev, D, N, L = self.dev, self.D, self.N, self.L
        M, Mp = R * N, _r64(R * N)
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        b16 = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=dev)
        Rp, Tp = _r64(R), _r64(R * self.tok)
        # operands of a weight gradient are allocated with their token dimension padded to 64 ZERO rows (never
        # written: every producer stops at row M); "*_full" is the padded tensor, the plain name its [:M] view
        pad = lambda rows, rp, cols: b16(rp, cols)
        full = dict(h1=[pad(M, Mp, D) for _ in range(L)], o=[pad(M, Mp, D) for _ in range(L)],
                    h2=[pad(M, Mp, D) for _ in range(L)], g=[pad(M, Mp, 4 * D) for _ in range(L)],
                    dxb=pad(M, Mp, D), dwide=pad(M, Mp, 4 * D), dqkv=pad(M, Mp, 3 * D),
                    dfeats=pad(R, Rp, 1024), c=pad(R, Rp, D), dtok=pad(R * self.tok, Tp, D),
                    patches=pad(R * self.tok, Tp, 3 * self.P_ * self.P_))
        b = dict(M=M, Mp=Mp, Rp=Rp, Tp=Tp, full=full,
                 x=[f32(M, D) for _ in range(2 * L + 1)],                      # residual stream snapshots
                 h1=[t[:M] for t in full["h1"]], qkv=[b16(M, 3 * D) for _ in range(L)],
                 o=[t[:M] for t in full["o"]], lse=[f32(R * self.H * N) for _ in range(L)],
                 h2=[t[:M] for t in full["h2"]], u=[b16(M, 4 * D) for _ in range(L)], g=[t[:M] for t in full["g"]],
                 c=full["c"][:R], feats=f32(R, 1024), logits=f32(R, self.nc), labels=torch.zeros(R, dtype=torch.int32, device=dev),
                 dx=f32(M, D), dxb=full["dxb"][:M], dwide=full["dwide"][:M], dqkv=full["dqkv"][:M], dnar=b16(M, D),
                 delta=f32(R * self.H * N), dfeats=full["dfeats"][:R], dc=b16(R, D),
                 dtok=full["dtok"][:R * self.tok], dtok32=f32(R * self.tok, D), patches=full["patches"][:R * self.tok],
                 dpos=f32(N, D),
                 # gradient operands of a block's four weight gradients, double-buffered by block parity: the weight
                 # gradients of block i run on a second stream while the main stream already writes block i-1's set
                 dy=[dict(dxb_fc2=pad(M, Mp, D), dxb_proj=pad(M, Mp, D), dwide=pad(M, Mp, 4 * D), dqkv=pad(M, Mp, 3 * D),
                          done=None) for _ in range(2)],
                 ws=f32(max(int(lib.yv_colsum_ws_floats(M, 4 * D)), int(lib.yv_layernorm_bwd_ws_floats(M, D)), 2 * R * 128) + 64),
                 ws_w=f32(int(lib.yv_colsum_ws_floats(M, 4 * D)) + 64))          # scratch of the column sums on the side stream
        if self.dtype == "mxfp8":
            # MX operands.  Row forms (GEMM A operands, consumed by the next GEMM on the main stream): one set per width.  Column
            # forms (weight-gradient operands, (C, Mq) with the tokens zero-padded to Mq = M rounded up to 128): the forward's
            # activations per block (read by backward), the gradients double-buffered by block parity like b["dy"]
            u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)
            Mq = r128(M)
            row = lambda C: (u8(M, C), u8(C // 128, Mq, 4))
            col = lambda C: (u8(C, Mq), u8(Mq // 128, r128(C), 4))
            b.update(Mq=Mq, rq={C: row(C) for C in (D, 3 * D, 4 * D)},
                     xc=[dict(h1=col(D), o=col(D), h2=col(D), g=col(4 * D)) for _ in range(L)])
            for S in b["dy"]:
                S.update(c_fc2=col(D), c_wide=col(4 * D), c_proj=col(D), c_qkv=col(3 * D))
        if self._tail:
            # the last block's compact cls-row operands; those that feed a weight gradient have Rp rows and a zero tail that nothing
            # writes.  The three gradient operands are this block's own (only one block uses them): no parity protocol
            b["tail"] = dict(o=b16(Rp, D), h2=b16(Rp, D), g=b16(Rp, 4 * D), u=b16(R, 4 * D), xmid=f32(R, D), xout=f32(R, D),
                             lse=f32(R * self.H), q=b["qkv"][L - 1][::N, :D], dxc=f32(R, D), dxb_fc2=b16(Rp, D),
                             dxb_proj=b16(Rp, D), dwide=b16(Rp, 4 * D), dnar=b16(R, D), do=b16(R, D))
        self._bufs[R] = b
        return b

    # ---- the three products of a block linear: the recipe (self.dtype) is chosen here and nowhere in the block bodies -----------
    # `lin` names the linear inside block i ("attn.qkv", ...).  `col` names the buffer that takes the column form of the quantised
    # operand, which the weight gradient reads (mxfp8 only; bf16 has no such form).  `cls` marks a compact cls-row operand: the
    # mxfp8 recipe runs those products in bf16 on the bf16 mirror.  `epi` is the epilogue: flags, res_f32, aux.
    def _quant(self, b: dict, x: torch.Tensor, col: Optional[tuple]):
        """bf16 (M, C) operand -> its row form (the shared A operand of width C) and, if `col`, its column form: one read."""
        q, s = b["rq"][x.shape[1]]
        quant_mxfp8_2d(x, q, s, *(col if col is not None else (None, None)), col_form=col is not None)
        return q, s

    def _product(self, b: dict, i: int, lin: str, x: torch.Tensor, out: torch.Tensor, col: Optional[str] = None,
                 cls: bool = False, **epi):
        """Forward product out = x . W^T + bias.  bf16: linear, or linear_ex where the epilogue has a residual source or an aux
        tensor.  mxfp8: x quantised (column form into b["xc"][i][col]), then linear_mxfp8_ex on the row-wise MX weight."""
        key = f"model.blocks.{i}.{lin}.weight"
        bias = self.p(f"model.blocks.{i}.{lin}.bias")
        if self.dtype == "mxfp8" and not cls:
            wq, ws = self.wmx[key][:2]
            linear_mxfp8_ex(*self._quant(b, x, b["xc"][i][col]), wq, ws, bias, out, **epi)
        else:
            (linear_ex if "res_f32" in epi or "aux" in epi else linear)(x, self.gemm_w[key][2], bias, out, **epi)

    def _dgrad(self, b: dict, S: dict, i: int, lin: str, dy: torch.Tensor, out: torch.Tensor, col: Optional[str] = None,
               cls: bool = False, **epi):
        """Data gradient out = dy . W.  bf16: linear / linear_ex on the transposed mirror.  mxfp8: dy quantised (column form into
        S[col]), then linear_mxfp8_ex on the MX W^T; cls rows: linear_nn on the master layout (the recipe has no transposed mirror)."""
        key = f"model.blocks.{i}.{lin}.weight"
        if self.dtype == "bf16":
            (linear_ex if "aux" in epi else linear)(dy, self.wt(key), None, out, **epi)
        elif cls:
            linear_nn(dy, self.gemm_w[key][2], out, **epi)
        else:
            wtq, wts = self.wmx[key][2:]
            linear_mxfp8_ex(*self._quant(b, dy, S[col]), wtq, wts, None, out, **epi)

    def _wgrad_bf16(self, dy: torch.Tensor, x: torch.Tensor, dw: torch.Tensor, **kw):
        """The bf16 weight-gradient launch: wgrad, or with wide_wgrad the routed wgrad_wide on the same operands."""
        if self.wide_wgrad:
            wgrad_wide(dy, x, dw, routed=True, **kw)
        else:
            wgrad(dy, x, dw, **kw)

    def _wgrad(self, b: dict, S: dict, i: int, w: str, dy: str, col: str, x: str, tail: Optional[dict] = None):
        """Weight gradient G[w] = dy^T . x of block i.  `dy` names the gradient operand in the parity set S (`col`: its column form),
        `x` the activation.  bf16: wgrad on the 64-row padded, zero-tailed operands.  mxfp8: wgrad_mxfp8 on the column forms.
        Operands that `tail` holds are compact cls rows: wgrad over their Rp rows, in both recipes."""
        dw = self._g2d(f"model.blocks.{i}.{w}")
        if tail is not None and dy in tail:
            self._wgrad_bf16(tail[dy], tail[x], dw, T=b["Rp"])
        elif self.dtype == "mxfp8":
            wgrad_mxfp8(*S[col], *b["xc"][i][x], dw)
        else:
            self._wgrad_bf16(S[dy], b["full"][x][i], dw)

    def _side_stream_epilogue(self, b: dict, S: dict, i: int, main, dwide: torch.Tensor, dqkv: torch.Tensor,
                              tail: Optional[dict] = None):
        """The end of every block's backward: its four weight gradients and the two bias gradients that are pure column sums (fc1,
        qkv).  Nothing on the data-gradient chain needs them, so they run on the side stream (own split-K workspace and column-sum
        scratch) under the next block's chain; the gradient buckets that become final with them are launched from that stream,
        i.e. after them.  S["done"] lets block i-2, which writes the same parity set, wait for these reads."""
        k = f"model.blocks.{i}."
        ev = torch.cuda.Event()
        ev.record(main)
        with torch.cuda.stream(self.s_w):
            self.s_w.wait_event(ev)
            colsum_bf16(dwide, self.g(k + "mlp.fc1.bias"), b["ws_w"])
            colsum_bf16(dqkv, self.g(k + "attn.qkv.bias"), b["ws_w"])
            for w, dy, col, x in BLOCK_WGRADS:
                self._wgrad(b, S, i, w, dy, col, x, tail)
            self.reducer.ready(self.off[k + "norm1.weight"])
            S["done"] = torch.cuda.Event()
            S["done"].record(self.s_w)

    def _attention_fwd(self, b: dict, i: int, R: int):
        """Block i's attention forward with the log2-sum-exp the backward needs."""
        if self.long_attn and self.N > 224:
            attention_long(b["qkv"][i], R, self.N, self.H, b["o"][i], lse=b["lse"][i])
        else:
            attention_train(b["qkv"][i], R, self.N, self.H, b["o"][i], b["lse"][i])

    def _attention_bwd(self, *args):
        """A block's attention backward (operands of attention_bwd): all three kernels write the same bits."""
        if self.short_attn_bwd and self.N <= 224:
            attention_bwd_short(*args)
        elif self.long_attn_bwd and self.N > 224:
            attention_bwd_long(*args)
        else:
            attention_bwd(*args)

    # ---- the full block (both recipes) ---------------------------------------------------------------------
    def _block_forward(self, b: dict, i: int, R: int):
        D, M = self.D, b["M"]
        p = lambda n: self.p(f"model.blocks.{i}.{n}")
        xin, xmid, xout = b["x"][2 * i:2 * i + 3]
        layernorm(xin, p("norm1.weight"), p("norm1.bias"), b["h1"][i], M, D, D, D)
        self._product(b, i, "attn.qkv", b["h1"][i], b["qkv"][i], col="h1")
        self._attention_fwd(b, i, R)
        self._product(b, i, "attn.proj", b["o"][i], xmid, col="o", flags=EPI_RES_F32, res_f32=xin)
        layernorm(xmid, p("norm2.weight"), p("norm2.bias"), b["h2"][i], M, D, D, D)
        self._product(b, i, "mlp.fc1", b["h2"][i], b["g"][i], col="h2", flags=EPI_GELU | EPI_SAVE_PRE, aux=b["u"][i])
        self._product(b, i, "mlp.fc2", b["g"][i], xout, col="g", flags=EPI_RES_F32, res_f32=xmid)

    def _block_backward(self, b: dict, S: dict, i: int, main, R: int):
        """The block's data-gradient chain on the main stream (b["dx"]: the gradient of its output, then of its input), then its
        weight gradients on the side stream.  The gradient operands live in the parity set S."""
        D, N, H, M = self.D, self.N, self.H, b["M"]
        p, g = (lambda n: self.p(f"model.blocks.{i}.{n}")), (lambda n: self.g(f"model.blocks.{i}.{n}"))
        xin, xmid, dx = b["x"][2 * i], b["x"][2 * i + 1], b["dx"]
        dxb_fc2, dxb_proj, dwide, dqkv = S["dxb_fc2"][:M], S["dxb_proj"][:M], S["dwide"][:M], S["dqkv"][:M]
        # MLP branch
        cast_colsum(dx, dxb_fc2, g("mlp.fc2.bias"), b["ws"])
        self._dgrad(b, S, i, "mlp.fc2", dxb_fc2, dwide, col="c_fc2", flags=EPI_GELU_BWD, aux=b["u"][i])
        self._dgrad(b, S, i, "mlp.fc1", dwide, b["dnar"], col="c_wide")
        layernorm_bwd(xmid, D, p("norm2.weight"), b["dnar"], D, M, D, dx, D, g("norm2.weight"), g("norm2.bias"), b["ws"])
        # attention branch
        cast_colsum(dx, dxb_proj, g("attn.proj.bias"), b["ws"])
        self._dgrad(b, S, i, "attn.proj", dxb_proj, b["dnar"], col="c_proj")
        self._attention_bwd(b["qkv"][i], b["o"][i], b["dnar"], b["lse"][i], R, N, H, dqkv, b["delta"])
        self._dgrad(b, S, i, "attn.qkv", dqkv, b["dnar"], col="c_qkv")
        layernorm_bwd(xin, D, p("norm1.weight"), b["dnar"], D, M, D, dx, D, g("norm1.weight"), g("norm1.bias"), b["ws"])
        self._side_stream_epilogue(b, S, i, main, dwide, dqkv)

    # ---- the last block on the cls rows (cls_tail=True, both recipes) ---------------------------------------
    def _tail_forward(self, b: dict, i: int, R: int):
        """Block L-1 forward: LN1 and the qkv product over every row (K and V of every token are needed), the rest on the R cls
        rows.  The residual rows are copied into the f32 output first, so that proj and fc2 use the in-place EPI_RES_F32 form."""
        D, N, H, M, T = self.D, self.N, self.H, b["M"], b["tail"]
        p = lambda n: self.p(f"model.blocks.{i}.{n}")
        xin = b["x"][2 * i]
        layernorm(xin, p("norm1.weight"), p("norm1.bias"), b["h1"][i], M, D, D, D)
        self._product(b, i, "attn.qkv", b["h1"][i], b["qkv"][i], col="h1")
        attention_cls_train(T["q"], b["qkv"][i], R, N, H, T["o"][:R], T["lse"])
        T["xmid"].copy_(xin[::N])
        self._product(b, i, "attn.proj", T["o"][:R], T["xmid"], cls=True, flags=EPI_RES_F32)
        layernorm(T["xmid"], p("norm2.weight"), p("norm2.bias"), T["h2"], R, D, D, D)
        self._product(b, i, "mlp.fc1", T["h2"][:R], T["g"][:R], cls=True, flags=EPI_GELU | EPI_SAVE_PRE, aux=T["u"])
        T["xout"].copy_(T["xmid"])
        self._product(b, i, "mlp.fc2", T["g"][:R], T["xout"], cls=True, flags=EPI_RES_F32)

    def _tail_backward(self, b: dict, S: dict, i: int, main, R: int):
        """Block L-1 backward.  b["tail"]["dxc"] holds the cls rows of the incoming gradient (every other row is zero): MLP branch,
        LN2 and proj on the R cls rows, attention_cls_bwd into the block's ordinary dqkv set, then the full-row end of the block
        (qkv data gradient, LN1 backward) and the side-stream epilogue with three of the four weight gradients on compact rows."""
        D, N, H, M, T = self.D, self.N, self.H, b["M"], b["tail"]
        p, g = (lambda n: self.p(f"model.blocks.{i}.{n}")), (lambda n: self.g(f"model.blocks.{i}.{n}"))
        xin, dx, dxc, dqkv = b["x"][2 * i], b["dx"], T["dxc"], S["dqkv"][:M]
        dxb_fc2, dxb_proj, dwide = T["dxb_fc2"][:R], T["dxb_proj"][:R], T["dwide"][:R]
        # MLP branch
        cast_colsum(dxc, dxb_fc2, g("mlp.fc2.bias"), b["ws"])
        self._dgrad(b, S, i, "mlp.fc2", dxb_fc2, dwide, cls=True, flags=EPI_GELU_BWD, aux=T["u"])
        self._dgrad(b, S, i, "mlp.fc1", dwide, T["dnar"], cls=True)
        layernorm_bwd(T["xmid"], D, p("norm2.weight"), T["dnar"], D, R, D, dxc, D, g("norm2.weight"), g("norm2.bias"), b["ws"])
        # attention branch: one query per crop; dK and dV for every key, zeros in the other rows' dQ
        cast_colsum(dxc, dxb_proj, g("attn.proj.bias"), b["ws"])
        self._dgrad(b, S, i, "attn.proj", dxb_proj, T["do"], cls=True)
        attention_cls_bwd(T["q"], b["qkv"][i], T["do"], T["lse"], R, N, H, dqkv)
        dx[::N].copy_(dxc)                                     # dx is zero elsewhere (backward zeroes it)
        self._dgrad(b, S, i, "attn.qkv", dqkv, b["dnar"], col="c_qkv")
        layernorm_bwd(xin, D, p("norm1.weight"), b["dnar"], D, M, D, dx, D, g("norm1.weight"), g("norm1.bias"), b["ws"])
        self._side_stream_epilogue(b, S, i, main, dwide, dqkv, tail=T)

    # ---- forward (activations kept) -------------------------------------------------------------------
    def forward(self, patches: torch.Tensor, R: int) -> torch.Tensor:
        b = self._buffers(R)
        D, N, tok, L = self.D, self.N, self.tok, self.L
        b["patches"].copy_(patches)                            # token-padded copy (operand of the patch-embed wgrad)
        patches = b["patches"]
        x0 = b["x"][0]
        cls_rows(self.p("model.cls_token").reshape(D), self.p("model.pos_embed").reshape(N, D), R, tok, D, x0)
        linear(patches, self.gemm_w["model.patch_embed.proj.weight"][2], self.p("model.patch_embed.proj.bias"), x0,
               flags=EPI_OUT_F32 | EPI_POSEMB, pos=self.p("model.pos_embed").reshape(N, D), tok=tok)
        for i in range(L):
            (self._tail_forward if i == L - 1 and self._tail else self._block_forward)(b, i, R)
        if self._tail:
            layernorm(b["tail"]["xout"], self.p("model.norm.weight"), self.p("model.norm.bias"), b["c"], R, D, D, D)
        else:
            layernorm(b["x"][2 * L], self.p("model.norm.weight"), self.p("model.norm.bias"), b["c"], R, D, N * D, D)
        linear(b["c"], self.w_head_pad, self.b_head_pad, b["feats"], flags=EPI_OUT_F32)
        w1t = self.p("fc.1.weight").t().contiguous()
        b["w1t"] = w1t
        wrapper_head(b["feats"], w1t, self.p("fc.1.bias"), self.p("fc.3.weight"), self.p("fc.3.bias"), R, self.nc,
                     b["logits"], b["labels"])
        return b["logits"]

    # ---- backward ---------------------------------------------------------------------------------------
    def backward(self, patches: torch.Tensor, labels: torch.Tensor, R: int) -> torch.Tensor:
        b = self._buffers(R)
        D, N, tok, L = self.D, self.N, self.tok, self.L
        self.reducer.reset()
        loss, dlogits = loss_fwd_bwd(b["logits"], labels)
        # ---- Network_Wrapper.fc + backbone head -----------------------------------------------------------
        # reducer.ready(offset): gradients at offsets >= offset are final; their all-reduce starts while backward continues
        head_bwd(b["feats"], b["w1t"], self.p("fc.1.bias"), self.p("fc.3.weight"), dlogits, R, self.nc,
                 self.g("fc.1.weight"), self.g("fc.1.bias"), self.g("fc.3.weight"), self.g("fc.3.bias"), b["dfeats"], b["ws"])
        self.reducer.ready(self.off["fc.1.weight"])
        colsum_bf16(b["dfeats"], b["ws"][:1024], b["ws"][1024:], rows=R)
        self.g("model.head.bias").copy_(b["ws"][:1000])
        self._wgrad_bf16(b["full"]["dfeats"][:, :1000], b["full"]["c"], self._g2d("model.head.weight"))
        linear_nn(b["dfeats"], self.w_head_pad, b["dc"])
        b["dx"].zero_()
        if self._tail:
            b["tail"]["dxc"].zero_()
            layernorm_bwd(b["tail"]["xout"], D, self.p("model.norm.weight"), b["dc"], D, R, D, b["tail"]["dxc"], D,
                          self.g("model.norm.weight"), self.g("model.norm.bias"), b["ws"])
        else:
            layernorm_bwd(b["x"][2 * L], N * D, self.p("model.norm.weight"), b["dc"], D, R, D, b["dx"], N * D,
                          self.g("model.norm.weight"), self.g("model.norm.bias"), b["ws"])
        self.reducer.ready(self.off["model.norm.weight"])
        # ---- transformer blocks, last to first -------------------------------------------------------------
        main = torch.cuda.current_stream()
        if self.s_w is None:
            self.s_w = torch.cuda.Stream()
        for i in reversed(range(L)):
            S = b["dy"][i & 1]                                 # gradient operands, double-buffered by block parity
            if S["done"] is not None:
                main.wait_event(S["done"])                     # block i+2's weight gradients have read this set
            (self._tail_backward if i == L - 1 and self._tail else self._block_backward)(b, S, i, main, R)
        main.wait_stream(self.s_w)
        # ---- embeddings -----------------------------------------------------------------------------------
        token_reduce(b["dx"], R, N, D, b["dpos"])
        self.g("model.pos_embed").copy_(b["dpos"].view(1, N, D))
        self.g("model.cls_token").copy_(b["dpos"][0].view(1, 1, D))
        b["dtok32"].copy_(b["dx"].view(R, N, D)[:, 1:, :].reshape(R * tok, D))          # drop the cls rows (copy only)
        cast_colsum(b["dtok32"], b["dtok"], self.g("model.patch_embed.proj.bias"), b["ws"])
        self._wgrad_bf16(b["full"]["dtok"], b["full"]["patches"], self._g2d("model.patch_embed.proj.weight"))
        return loss

    # ---- optimizer ----------------------------------------------------------------------------------------
    def optimizer_step(self, lr: float):
        import torch.distributed as dist
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        self.reducer.finish()
        sgd_step(self.P, self.G, self.Mo, lr, self.momentum, self.wd, first=self.steps == 0, grad_scale=1.0 / world,
                 mirror=self.P16)
        self.steps += 1
        self.refresh_working_copies()

    def step(self, patches: torch.Tensor, labels: torch.Tensor, lr: float):
        """One fine-tune step; `patches` (R*tok, 3*P*P) bf16 patch-major crops, `labels` (R) int32.
        Returns (loss (1,) f32 device tensor, logits (R,nc))."""
        R = labels.shape[0]
        logits = self.forward(patches, R)
        loss = self.backward(patches, labels, R)
        self.optimizer_step(lr)
        return loss, logits
