"""fp64 reference and componentwise worst-case error bounds of the attention backward kernels (a helper module, like
mx_train_emulation.py; test_attn_bwd_reference_cpu.py proves the gate on the CPU, test_gpu_attn_bwd_bound.py applies it to the kernels).

The reference is a function of the OPERANDS a kernel is given (qkv, out, dout, lse), not of a forward pass: `operands()` builds
out = bf16(fp64 forward output) and lse = f32(fp64 log2-sum-exp of the scaled scores) on the CPU, so the bf16 rounding of O is part of
the input and no forward kernel takes part in a backward check.  With c = scale * log2(e), in fp64:

    P = exp2(c Q K^T - lse)   delta = sum_d dO O   dP = dO V^T   dS = P (dP - delta) scale   dQ = dS K   dK = dS^T Q   dV = P^T dO

The gate is |got - ref| <= GATE * B for EVERY element, GATE = 1.01, with B a first-order worst-case bound built from two constants
only: U = 2^-8, the unit roundoff of round-to-nearest bf16 (8 significant bits), and G64 = 64 * 2^-24, an f32 dot product of 64 terms
in any order (EPS = 2^-24 is one f32 rounding).  The 1 % is for the second-order terms (U^2 = 1.5e-5 relative).  Nothing is fitted.

yv_attention_bwd, yv_attention_bwd_long and yv_attention_bwd_short compile ONE text of the element-wise expressions, casts and MFMA
order, csrc/attention_bwd_core.h (owner_query, to_ds, to_p_ds, dq_group, dkv_group, store_head_row; the three .hip files hold blocking
and staging only), and are bit-equal by their own tests and tests/golden/attn_bwd_bits.json.  Lines of that header:
  * score argument (lines 163, 136 / 191, 147: MFMA f32 accumulation of S, the f32 lse, one multiply, one subtract, exp2f):
        delta_arg = c G64 (|Q| |K|^T) + 2^-23 (|c S| + |lse| + 1)
  * P:   E_P = U P + P delta_arg ln2.  The U term is the cast of P to bf16 before P^T dO (line 201, `fp[j] = (__bf16)sv[..]`).
  * dS:  E_S = U |dS| + |dS| (delta_arg ln2 + 4 EPS) + P scale G64 (|dO| |V|^T + sum_d |dO O|).  U: the cast of dS to bf16 (lines 173
         and 201, `fp[j] = (__bf16)s[..]`, `fs[j] = (__bf16)dp[..]`); 4 EPS: the subtract and the two multiplies of lines 137 / 149; the
         last term is the f32 cancellation in dP - delta (dP: MFMA, line 164 / 192; delta: lines 112-114) and dominates where the softmax
         is peaked - without it the bound is not a bound.
  * outputs (f32 MFMA accumulation over N keys / queries, lines 176, 204, 205, then pack_bf16x2, RNE, line 217):
        B_dQ = E_S |K| + N EPS (|dS| |K|) + U |dQ|     B_dK = E_S^T |Q| + N EPS (|dS|^T |Q|) + U |dK|
        B_dV = E_P^T |dO| + N EPS (P^T |dO|) + U |dV|  B_delta = G64 sum_d |dO O|   (64 exact bf16 x bf16 products summed in f32)

yv_attention_cls_bwd (csrc/attention_cls_train.hip, f32 throughout, no bf16 operand cast, reads no O):
  * p_n = exp2(dot8(q, k_n) c - lse) (line 158): E_p = p delta_arg ln2 - no U p term.   dp_n = dot8(dO, v_n) (line 159): G64 |dO| |v_n|.
  * delta = sum_n p_n dp_n, made by the kernel (lines 162, 169-172: ceil(N / 32) terms per 8-lane group, then 32 groups, one product):
        E_delta = sum_n (E_p |dp_n| + p_n G64 |dO| |v_n|) + (ceil(N / 32) + 33) EPS sum_n |p_n dp_n|
  * ds_n = p_n (dp_n - delta) scale (line 183): E_s = E_p |dp_n - delta| scale + p_n scale (G64 |dO| |v_n| + E_delta) + 4 EPS |ds_n|
    - no U |dS| term.
  * dk_n = ds_n q (line 187), dv_n = p_n dO (line 165), one f32 product each, then pack_bf16x8 (RNE, lines 166, 190):
        B_dK = E_s |q| + (U + EPS) |dk|     B_dV = E_p |dO| + (U + EPS) |dv|
    dq = sum_n ds_n k_n (lines 188, 195-207: per group, three shuffles, four waves):
        B_dQ = E_s |K| + (ceil(N / 32) + 8) EPS (|ds| |K|) + U |dq|
    The Q third of every row n >= 1 is exactly zero (line 191): reference 0, bound 0.

yv_attention_train (csrc/attention.hip, attention_kernel lines 124-251 and attention_pipe_kernel lines 470-519) and
yv_attention_cls_train (attention_cls_train.hip lines 72-96): p = exp2(c s - mb) with mb the scaled row maximum, so the shift is
|mb| <= |lse| + log2 N in delta_arg.  The row sum l adds the f32 p (attention.hip:151, 214), the product P V takes p cast to bf16
(lines 157, 233, 476), and O = (sum p V) / l is rounded to bf16 (line 290):
        B_out = U (|O| + P |V|) + (P delta_arg ln2) |V| + (sum_k P_k delta_arg_k ln2 + (2 N + 8) EPS) (P |V|)
    The last group is the error of the normaliser l (the terms' own errors and their f32 summation) and of the f32 accumulation over
    the keys, the rescales by alpha (lines 139-144, 205-223: the same alpha multiplies o and l) and the division.
        B_lse = (N + 8) EPS log2(e) + 2^-23 |lse|
    (N + 8) EPS: worst-case sequential f32 summation of N terms in [0, 1], and log2f; 2^-23 |lse|: mb = m c, the final add (line 250) and
    f32 storage.  NOT in B_lse: the error the terms of l carry from the f32 accumulation of the scores (attention.hip:124, 184;
    attention_cls_train.hip:72-76), sum_k P_k delta_arg_k in the worst case.  The worst-case G64 |Q| |K|^T would widen B_lse tenfold on
    the peaked data; the bound is kept as tight as stated (the kernels reach 0.41 and 0.26 of it on the case list), and if a case ever exceeds it this
    is the first term to weigh.
"""
import functools
import math

import torch

U = 2.0 ** -8                      # unit roundoff of round-to-nearest bf16
EPS = 2.0 ** -24                   # unit roundoff of f32
G64 = 64 * EPS                     # an f32 dot product of 64 terms, any order
GATE = 1.01                        # derived (second-order terms), not fitted
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
SCALE = 0.125                      # 64 ** -0.5, the kernels' default

# (R, N, H): every NT = ceil(N / 32) instantiation of yv_attention_bwd at both of its edges, the multi-tile seams, R, H > 1, an odd H
BWD_SHAPES = [(2, 1, 1), (1, 31, 2), (2, 32, 1), (1, 33, 3),
              (2, 64, 1), (1, 65, 2), (1, 96, 1), (2, 97, 1),
              (1, 128, 2), (1, 129, 1), (1, 160, 1), (2, 161, 2),
              (1, 192, 1), (1, 193, 1), (2, 197, 3), (1, 224, 1), (1, 225, 2), (1, 256, 1),
              (1, 257, 2), (1, 511, 1), (1, 512, 1), (1, 513, 1), (2, 785, 2)]
CLS_SHAPES = [(2, 1, 1), (2, 5, 2), (1, 33, 3), (2, 197, 2), (1, 257, 1), (2, 785, 2)]
KINDS = ("flat", "peaked")


def bf(t):
    return t.to(torch.bfloat16)


def heads(x, R, N, H):
    """(R*N, H*64) -> (R, H, N, 64)"""
    return x.reshape(R, N, H, 64).permute(0, 2, 1, 3)


def rows(x, R, N, H):
    """(R, H, N, 64) -> (R*N, H*64)"""
    return x.permute(0, 2, 1, 3).reshape(R * N, H * 64)


def split_qkv(qkv, R, N, H, dtype=torch.float64):
    """(R*N, 3*H*64) -> q, k, v, each (R, H, N, 64)"""
    t = qkv.to(dtype).view(R, N, 3, H, 64)
    return tuple(t[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def _arg_error(q, k, S, c, shift_abs):
    """delta_arg: the absolute error of the f32 exponent c S - shift, exp2f's own error included (in units of the argument)."""
    return c * G64 * (q.abs() @ k.abs().mT) + 2.0 ** -23 * ((c * S).abs() + shift_abs + 1.0)


def worst(got, ref, bound):
    """-> (max |got - ref| / bound, flat index of it); 0 / 0 counts as 0, anything non-finite or x / 0 as inf."""
    diff = (got.double() - ref).abs().reshape(-1)
    b = bound.reshape(-1)
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / b)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return float(ratio[i]), i


# ------------------------------------------------------------------------------------------------ forward
def fwd_reference(qkv, R, N, H, scale=SCALE):
    """fp64 forward of bf16 qkv -> dict: out (R*N, D), lse (R*H*N) [log2 domain], and the bounds b_out, b_lse of yv_attention_train
    (module docstring)."""
    q, k, v = split_qkv(qkv, R, N, H)
    c = scale * LOG2E
    S = q @ k.mT
    cS = c * S
    m = cS.max(-1, keepdim=True).values
    lse = m + torch.log2(torch.exp2(cS - m).sum(-1, keepdim=True))
    P = torch.exp2(cS - lse)
    O = P @ v
    w = P * _arg_error(q, k, S, c, lse.abs() + math.log2(N))
    PV = P @ v.abs()
    b_out = U * (O.abs() + PV) + LN2 * (w @ v.abs()) + (LN2 * w.sum(-1, keepdim=True) + (2 * N + 8) * EPS) * PV
    b_lse = (N + 8) * EPS * LOG2E + 2.0 ** -23 * lse.abs()
    return {"out": rows(O, R, N, H), "lse": lse.reshape(-1), "b_out": rows(b_out, R, N, H), "b_lse": b_lse.reshape(-1)}


# ------------------------------------------------------------------------------------------------ backward
def bwd_reference(qkv, out, dout, lse, R, N, H, scale=SCALE):
    """fp64 backward of the operands -> dict: dqkv (R*N, 3D) [dQ | dK | dV], delta (R*H*N) and their bounds b_dqkv, b_delta."""
    q, k, v = split_qkv(qkv, R, N, H)
    o, do = heads(out.double(), R, N, H), heads(dout.double(), R, N, H)
    l = lse.double().view(R, H, N, 1)
    c = scale * LOG2E
    S = q @ k.mT
    P = torch.exp2(c * S - l)
    delta = (do * o).sum(-1, keepdim=True)
    dabs = (do * o).abs().sum(-1, keepdim=True)
    dP = do @ v.mT
    dPabs = do.abs() @ v.abs().mT
    dS = P * (dP - delta) * scale
    dQ, dK, dV = dS @ k, dS.mT @ q, P.mT @ do
    da = _arg_error(q, k, S, c, l.abs())
    e_p = U * P + P * da * LN2
    e_s = U * dS.abs() + dS.abs() * (da * LN2 + 4 * EPS) + P * scale * G64 * (dPabs + dabs)
    b_dq = e_s @ k.abs() + N * EPS * (dS.abs() @ k.abs()) + U * dQ.abs()
    b_dk = e_s.mT @ q.abs() + N * EPS * (dS.abs().mT @ q.abs()) + U * dK.abs()
    b_dv = e_p.mT @ do.abs() + N * EPS * (P.mT @ do.abs()) + U * dV.abs()
    cat = lambda a, b, cc: torch.cat([rows(a, R, N, H), rows(b, R, N, H), rows(cc, R, N, H)], 1)
    return {"dqkv": cat(dQ, dK, dV), "b_dqkv": cat(b_dq, b_dk, b_dv), "delta": delta.reshape(-1), "b_delta": (G64 * dabs).reshape(-1)}


def cls_bwd_reference(q, qkv, dout, lse, R, N, H, scale=SCALE):
    """fp64 backward of the cls query: q (R, D) bf16 (any stride), dout (R, D), lse (R*H) -> dict: dqkv (R*N, 3D) with dQ in the cls
    rows and zeros in the Q third of the others, and b_dqkv, the f32-only bound of yv_attention_cls_bwd (module docstring)."""
    _, k, v = split_qkv(qkv, R, N, H)
    q0 = q.double().reshape(R, H, 1, 64)
    do = dout.double().reshape(R, H, 1, 64)
    l = lse.double().view(R, H, 1, 1)
    c = scale * LOG2E
    S = q0 @ k.mT                                                    # (R, H, 1, N)
    P = torch.exp2(c * S - l)
    e_p = P * _arg_error(q0, k, S, c, l.abs()) * LN2
    dP = do @ v.mT
    dPabs = do.abs() @ v.abs().mT
    trips = (N + 31) // 32
    delta = (P * dP).sum(-1, keepdim=True)
    e_delta = (e_p * dP.abs() + P * G64 * dPabs).sum(-1, keepdim=True) + (trips + 33) * EPS * (P * dP).abs().sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    e_s = e_p * (dP - delta).abs() * scale + P * scale * (G64 * dPabs + e_delta) + 4 * EPS * dS.abs()
    dK, dV, dQ = dS.mT * q0, P.mT * do, dS @ k                        # (R, H, N, 64) x 2, (R, H, 1, 64)
    b_dk = e_s.mT * q0.abs() + (U + EPS) * dK.abs()
    b_dv = e_p.mT * do.abs() + (U + EPS) * dV.abs()
    b_dq = e_s @ k.abs() + (trips + 8) * EPS * (dS.abs() @ k.abs()) + U * dQ.abs()

    def q_third(x):                                                  # (R, H, 1, 64) -> (R*N, D), zeros outside the cls rows
        full = torch.zeros(R, H, N, 64, dtype=torch.float64)
        full[:, :, :1] = x
        return rows(full, R, N, H)
    return {"dqkv": torch.cat([q_third(dQ), rows(dK, R, N, H), rows(dV, R, N, H)], 1),
            "b_dqkv": torch.cat([q_third(b_dq), rows(b_dk, R, N, H), rows(b_dv, R, N, H)], 1)}


# ------------------------------------------------------------------------------------------------ cases
def _seed(R, N, H, kind):
    return ((R * 1009 + N) * 13 + H) * 2 + KINDS.index(kind)


@functools.lru_cache(maxsize=None)
def operands(R, N, H, kind):
    """The operands of one case, all bf16-representable (lse f32), seeded per shape and kind, on the CPU; read-only by agreement.
    flat: randn; peaked: Q and K x 2.5 (a few keys carry a row: dS is large and dP - delta cancels).  V gets + 0.75 and dO + 0.5 in
    both, so delta is far from zero (zero-mean dO makes delta ~ 0 and hides its errors).
    -> dict: qkv, dout, out = bf16(fp64 forward), lse = f32(fp64 log2-sum-exp), fwd = fwd_reference(qkv)."""
    g = torch.Generator().manual_seed(_seed(R, N, H, kind))
    D = H * 64
    t = torch.randn(R * N, 3 * D, generator=g)
    if kind == "peaked":
        t[:, :2 * D] *= 2.5
    t[:, 2 * D:] += 0.75
    qkv = bf(t)
    dout = bf(torch.randn(R * N, D, generator=g) + 0.5)
    fwd = fwd_reference(qkv, R, N, H)
    return {"qkv": qkv, "dout": dout, "out": bf(fwd["out"]), "lse": fwd["lse"].float(), "fwd": fwd}


@functools.lru_cache(maxsize=None)
def bwd_case(R, N, H, kind):
    """operands(...) plus ref = bwd_reference of them."""
    ops = dict(operands(R, N, H, kind))
    ops["ref"] = bwd_reference(ops["qkv"], ops["out"], ops["dout"], ops["lse"], R, N, H)
    return ops


@functools.lru_cache(maxsize=None)
def cls_case(R, N, H, kind):
    """The cls-query case on the qkv of operands(...): dout (R, D), lse (R*H) of query 0 and its forward bounds, ref = cls_bwd_reference."""
    ops = operands(R, N, H, kind)
    D = H * 64
    g = torch.Generator().manual_seed(_seed(R, N, H, kind) + 1000003)
    dout = bf(torch.randn(R, D, generator=g) + 0.5)
    pick = lambda x: x.view(R, H, N)[:, :, 0].reshape(-1)
    fwd = ops["fwd"]
    lse = pick(fwd["lse"]).float()
    return {"qkv": ops["qkv"], "dout": dout, "lse": lse, "lse64": pick(fwd["lse"]), "b_lse": pick(fwd["b_lse"]),
            "ref": cls_bwd_reference(ops["qkv"][::N, :D], ops["qkv"], dout, lse, R, N, H)}


def thirds(D):
    return (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D)))


def ratios(got_dqkv, ref, D):
    """worst |got - ref| / bound per gradient third -> {"dq": r, "dk": r, "dv": r}, and the element of each as (row, column)"""
    out, where = {}, {}
    for name, sl in thirds(D):
        r, i = worst(got_dqkv[:, sl], ref["dqkv"][:, sl], ref["b_dqkv"][:, sl])
        out[name], where[name] = r, (i // D, i % D)
    return out, where
