"""fp64 references, derived worst-case error bounds, case lists and f32 CPU emulations of the HBM-bound glue kernels of the detector
trainer (a helper module, like vit_glue_reference.py; test_yolo_glue_reference_cpu.py proves the gates on the CPU,
test_gpu_yolo_glue.py applies them to the kernels): the BatchNorm statistics, BN + SiLU forward and backward
(csrc/yolo_train.hip), the exact kernels yv_view_op / yv_maxpool5_bwd / yv_im2col3 / yv_conv_weight_dgrad / yv_blob_nhwc8 /
yv_sppf_pool, and yv_detect_loss (csrc/yolo_loss.hip).

Every reference is a function of the OPERANDS the kernel is given (yv_bn_act_fwd / _bwd get mean and rstd as operands: their
references do not depend on yv_bn_stats).  Three kinds of check, and nothing is fitted to a kernel's output:

A. DERIVED BOUND, gate |got - ref| <= GATE * B for EVERY element, GATE = 1.01 (second-order terms), B from EPS = 2^-24 (one f32
rounding), U = 2^-8 (round-to-nearest bf16), EPS64 = 2^-53 and the kernel's own lines.  The library is built with
-ffp-contract=off and correctly rounded division and square root.  Rules (S) and (P) of vit_glue_reference.py:
  (S) a sum whose every term passes through at most d additions is off by at most d * EPS * sum|x_i|;
  (P) a product of factors known to +-d_i is off by at most prod(|f_i| + d_i) - prod|f_i| (not linearised), plus EPS of the
      result per multiplication.

Two-stage channel sums (chan_reduce_kernel, yolo_train.hip:55-127; chunk_sums 131-143).  chunks_for (421-427) cuts the T rows into
chunks of rows_per_chunk rows; with rp = 256 / (C / 8) row lanes a lane adds rows lane, lane + rp, ... of its chunk in increasing
order (lines 97-113: the four-rows-per-trip loop and its tail keep that order): ceil(rows_per_chunk / rp) f32 additions; the rp
lanes are added serially in f32 (line 124): rp more.  The second stage adds every 32nd chunk and then the 32 lanes in double
(lines 136, 142): ceil(chunks / 32) + 32 double additions.
    d1 = ceil(rows_per_chunk / rp) + rp        d2 = ceil(chunks / 32) + 32
    d_sum(x) = (d1 EPS + d2 EPS64) sum_r |x_r|
The bf16 operand z is exact in f32 and so is z * z (two 8-bit significands: line 78 rounds only in the additions).

yv_bn_stats (bn_stats_final_kernel, 145-164; m, var in double), s = sum z, ss = sum z^2, eps and momentum the f32 values passed:
    d_m    = d_sum(z) / T + EPS64 |m|                          B_mean = d_m + EPS |mean|                       (lines 154, 157)
    d_var  = d_sum(z^2) / T + ((|m| + d_m)^2 - m^2) + 4 EPS64 (ss / T + m^2)                                   (line 155, rule (P))
    The CANCELLATION of ss / T - m^2 is in d_var: for |m| >> std it is of the order of var itself, so rstd is NOT linearised:
    the computed variance lies in [max(var - d_var, 0), var + d_var] (the clamp of line 156 cannot move it away from var >= 0)
    B_rstd = max(1 / sqrt(max(var - d_var, 0) + eps) - rstd, rstd - 1 / sqrt(var + d_var + eps)) + EPS / sqrt(max(var - d_var, 0) + eps)
    B_run_mean = momentum d_m + EPS |run_mean|          B_run_var = momentum f d_var + EPS |run_var|,  f = T / (T - 1), 1 at T = 1
    (lines 160-162: torch's unbiased variance in the running estimate).  bn_stats_accuracy() gives B_rstd / rstd.

sigmoid_f (line 31) is 1 / (1 + __expf(-x)).  __expf scales its argument by log2(e) and takes the hardware exponential: one
rounding of the scaled argument is |x| EPS relative in the result; the hardware exponential is charged EXP_ULPS = 4 ulp = 8 EPS.
THIS FIGURE IS AN ASSUMPTION: no ISA text available to this project states the accuracy of v_exp_f32.  It is small against U for the
bf16 outputs and enters dgamma / dbeta only.  With the argument known to +-d_u:
    rel_e = |u| EPS + 2 EXP_ULPS EPS + d_u         d_sg = sg ((1 - sg) rel_e + 2 EPS)       (1 + e and the division: one EPS each)

yv_bn_act_fwd (bn_act_kernel<false>, lines 232-235):  u = gamma ((z - mean) rstd) + beta
    d_u = 3 EPS |gamma xhat| + EPS |u|               v = u (act 0), d_v = d_u;   v = u sg (act 1), rule (P) + EPS |v|
    no shortcut:  ref = v,                B_a = U |v| + d_v
    shortcut:     the kernel ROUNDS TWICE, bf16(bf16(v) + res) (line 234), and so does the reference: ref = bf16(v) + res with v in
                  fp64, B_a = U |ref| + EPS |ref| + d_v, plus one bf16 step of v for the elements whose v lies within d_v of a
                  rounding tie of bf16 (there the f32 kernel may round to the other neighbour).  A kernel that adds the shortcut
                  before the first rounding is off by up to U |v| and falls outside where the shortcut cancels the activation.

yv_bn_act_bwd (chan_reduce_kernel<1> lines 83-92, bn_bwd_final_kernel 178-190, bn_act_kernel<true> 242-250), d = da:
    xhat = (z - mean) rstd: d_xh = 2 EPS |xhat|;  u as above from xhat;  act 1: gr = d sg (1 + u (1 - sg)) by rule (P) through
    om = 1 - sg, u om, 1 + u om, sg (..), d (..) with one EPS each;  act 0: gr = d exactly.
    dbeta = sum gr, dgamma = sum gr xhat (line 91):
    B_dbeta  = sum d_gr + (d1 EPS + d2 EPS64) sum (|gr| + d_gr) + EPS |dbeta|
    B_dgamma = sum d_(gr xhat) + (d1 EPS + d2 EPS64) sum (|gr xhat| + d_(gr xhat)) + EPS |dgamma|
    k1 = f32(dbeta / T), k2 = f32(dgamma / T) (lines 188-189; 0 without batch statistics): d_k = (B - EPS |.|) / T + EPS |k|
    dz = bf16(sc ((gr - k1) - xhat k2)), sc = gamma rstd (lines 217, 249):
    d_t = d_gr + d_k1 + d_(xhat k2) + EPS |gr - k1| + EPS |t|          B_dz = U |dz| + |sc| d_t + 2 EPS |dz|

B. EXACT (bit for bit): operands are small integers that bf16 holds and every sum stays below 256, the references are written with
plain indexing below.  Also exact: the statistics of small-integer z (every f32 partial sum is an integer below 2^24, the double
stage is exact, the finaliser's formulas evaluated in numpy float64 in its order and rounded once), dbeta with act 0 and integer
da, dz with frozen statistics, act 0 and gamma rstd a power of two, and two calls on the same inputs.
NOT TESTED: the 64-bit-index instantiations of view_op_kernel / im2col3_kernel (they need 2^31 channel groups, 32 GB) and
gt_counts > G in yv_detect_loss (the caller's contract).

C. yv_detect_loss: DECISIONS EXACTLY, VALUES BY A MEASURED CONSTANT.  oracle/yolo_train.py does not run in double (its anchors
and the DFL projection are f32), so detect_loss_reference restates the loss from the operands in any dtype; in f32 it agrees with
oracle.yolo_train.detection_loss (CPU test), in f64 it is the reference.  Labels are clamped to [0, nc) as the kernel does
(yolo_loss.hip:131, 273).
Discrete decisions and why the f32 kernel must take them as the fp64 reference does:
  * anchor inside a box (line 125-127, 157-158) and the DFL bin floor(t) (308-310): every ground-truth coordinate of the case list
    is a multiple of 1/4 pixel (asserted), so px - x1, x / stride and ax - x / stride are EXACT in f32: the same numbers on both
    sides.  Box edges through anchor centres give dm = 0 exactly: outside (`>`); t an exact integer gives wl = 1 exactly.
  * top-10 per box (142-184) and the claimant with the highest overlap (187-203): either an exact tie by construction - metric
    exactly 0 on both sides (a class logit <= -120: __expf overflows, score 0, the reference flushes it too; or CIoU <= -CIOU_ERR:
    clamped to 0) or two identical boxes (identical operands) - decided by ascending index, or a margin: with CIOU_ERR = 1e-5 the
    assumed absolute f32 error of a CIoU value (inputs below 1000 pixels; the f32 evaluation of this file is within 2e-6) a
    metric lies in [sqrt(sc) max(iou - CIOU_ERR, 0)^6 (1 - 1e-5), sqrt(sc) (iou + CIOU_ERR)^6 (1 + 1e-5)]: every chosen anchor's lower
    end is above every other inside anchor's upper end; the two best overlaps of a contested anchor differ by more than 2 CIOU_ERR.
  * the branches of the CIoU gradient (75-79): |p_i - t_i| and the intersection's width and height are at least BRANCH_MARGIN = 1e-4
    grid units from 0 for every positive (the f32 error of a decoded coordinate is below 16 * 20 EPS = 2e-5).
  * a positive's weight is exactly 0 (metric 0) or at least 1e-12, so `dbox row non-zero` is `fg and weight > 0`.
loss_case draws by seed until all of this holds and asserts it; no anchor is left out of any comparison.
Values: |got - ref| <= K EPS (|ref| + max|ref| over the element's row) (the 64 box logits of an anchor, its ncp class logits, the
scalar itself), K = 8 * max(1, M) with M the worst |f32 - f64| / (EPS * scale) of THIS FILE's formulas evaluated in f32 with torch
over the whole case list: LOSS_M below, measured on the CPU and asserted there.  The factor 8 covers the kernel's __expf / __logf
and its summation order against libm's and torch's.
"""
import functools

import numpy as np
import torch

from vit_glue_reference import EPS, GATE, U, bf, int_tensor, lane_chain, worst  # noqa: F401  (re-exported to the tests)

EPS64 = 2.0 ** -53
EXP_ULPS = 4                       # ASSUMED accuracy of the hardware exponential behind __expf (module docstring)
NAN_ROWS = 2                       # input rows past T, all NaN
BN_EPS, BN_MOMENTUM = 1e-3, 0.03
ACT_ROWS_PER_LANE = 16             # yolo_train.hip:204
SENTINEL = -24576.0                # bf16-representable; no result of these cases comes near it


def f32v(x):
    """the value of python float x after rounding to f32, as a python float (what the kernel receives for a `float` argument)"""
    return float(torch.tensor(x, dtype=torch.float32))


def chunks_for(T):
    """yolo_train.hip:421-427 -> (chunks, rows_per_chunk)"""
    chunks = min((T + 255) // 256, 2048)
    rpc = (T + chunks - 1) // chunks
    return (T + rpc - 1) // rpc, rpc


def bn_ws_floats(T, C):
    return chunks_for(max(T, 1))[0] * 2 * C + 2 * C


def row_lanes(C):
    return 256 // (C // 8)


def _sum_rel(T, C):
    """d1 EPS + d2 EPS64 of the module docstring"""
    chunks, rpc = chunks_for(T)
    rp = row_lanes(C)
    return ((rpc + rp - 1) // rp + rp) * EPS + ((chunks + 31) // 32 + 32) * EPS64


# ------------------------------------------------------------------------------------------------ A: cases
def _bn_ts(C):
    rp = row_lanes(C)
    return sorted({1, max(rp - 1, 1), rp, rp + 1, 4 * rp - 1, 4 * rp, 4 * rp + 1, 16 * rp - 1, 16 * rp + 1, 257})


# (C, T, kind): every T class at C = 8 (256 row lanes), 24 (85 lanes, one idle thread) and 1024 (2 lanes); two chunks (257);
# 34 chunks (8449 at C = 16: two trips of the second stage's lanes); past the 2048-chunk cap (524289: 2041 chunks of 257 rows)
BN_CASES = [(C, T, "rand") for C in (8, 24, 1024) for T in _bn_ts(C)] + \
           [(48, 4 * 42 + 1, "rand"), (48, 257, "rand"), (256, 16 * 8 + 1, "rand"), (256, 257, "rand"),
            (8, 257, "values"), (24, 4 * 85 + 1, "values"), (1024, 33, "values"), (16, 8449, "rand"), (8, 524289, "rand")]
BN_BIG = {(16, 8449, "rand"), (8, 524289, "rand")}                     # run with one option set only
BN_OPTS = [(act, res) for act in (0, 1) for res in (False, True)]      # forward: activation, shortcut
BN_BWD_OPTS = [(act, bs) for act in (0, 1) for bs in (1, 0)]           # backward: activation, batch statistics
VALUE_CHANNELS = {"const": 0, "ratio8": 1, "ratio64": 2, "u+30": 3, "u-30": 4}


@functools.lru_cache(maxsize=None)
def bn_case(C, T, kind="rand", exact=False):
    """Operands on the CPU, read-only by agreement -> dict: z, da, res (T, C) f32 holding bf16 values, gamma, beta, rm0, rv0 (C).
    values: channel 0 constant 1.5 (var 0), channel 1 mean 8 std 1, channel 2 mean 64 std 1 (|mean| / std of 8 and 64), channels
    3 / 4 beta +-30 (the SiLU tails).  exact: integers in [-8, 8], gamma rstd = 2 and mean = 1 for the frozen-statistics case."""
    g = torch.Generator().manual_seed((C * 8209 + T) * 4 + ("rand", "values").index(kind) * 2 + exact)
    if exact:
        return {"z": int_tensor((T, C), g), "da": int_tensor((T, C), g), "res": int_tensor((T, C), g), "gamma": torch.full((C,), 2.0),
                "beta": int_tensor((C,), g), "rm0": int_tensor((C,), g), "rv0": int_tensor((C,), g, 0, 8)}
    z = torch.randn(T, C, generator=g) * 1.5 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    if kind == "values":
        z[:, 0] = 1.5
        z[:, 1] = 8 + torch.randn(T, generator=g)
        z[:, 2] = 64 + torch.randn(T, generator=g)
        gamma[3:5] = 0.5
        beta[3], beta[4] = 30.0, -30.0
    return {"z": bf(z).float(), "da": bf(torch.randn(T, C, generator=g)).float(), "res": bf(torch.randn(T, C, generator=g)).float(),
            "gamma": gamma, "beta": beta, "rm0": torch.randn(C, generator=g) * 0.1, "rv0": 1 + 0.1 * torch.rand(C, generator=g)}


# ------------------------------------------------------------------------------------------------ A: references and bounds
def bn_stats_reference(z, rm0=None, rv0=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """z (T, C) -> dict in fp64: mean, rstd, run_mean, run_var (the running pair only with rm0 / rv0) and b_<name>; var, d_var."""
    z = z.double()
    T, C = z.shape
    eps, mom, rel = f32v(eps), f32v(momentum), _sum_rel(T, C)
    m = z.sum(0) / T
    var = ((z - m) ** 2).sum(0) / T
    ss_t = (z * z).sum(0) / T
    d_m = rel * z.abs().sum(0) / T + EPS64 * m.abs()
    d_var = rel * ss_t + ((m.abs() + d_m) ** 2 - m * m) + 4 * EPS64 * (ss_t + m * m)
    rstd = 1 / torch.sqrt(var + eps)
    r_hi, r_lo = 1 / torch.sqrt((var - d_var).clamp(min=0) + eps), 1 / torch.sqrt(var + d_var + eps)
    out = {"mean": m, "b_mean": d_m + EPS * m.abs(), "rstd": rstd, "b_rstd": torch.maximum(r_hi - rstd, rstd - r_lo) + EPS * r_hi,
           "var": var, "d_var": d_var}
    if rm0 is not None:
        f = T / (T - 1) if T > 1 else 1.0
        out["run_mean"] = (1 - mom) * rm0.double() + mom * m
        out["run_var"] = (1 - mom) * rv0.double() + mom * var * f
        out["b_run_mean"] = mom * d_m + EPS * out["run_mean"].abs() + 4 * EPS64 * (rm0.double().abs() + m.abs())
        out["b_run_var"] = mom * f * d_var + EPS * out["run_var"].abs() + 4 * EPS64 * (rv0.double().abs() + var * f)
    return out


def bn_stats_accuracy(z, channel):
    """-> (|mean| / std, B_rstd / rstd) of one channel: how much of rstd the finaliser's ss / T - m^2 keeps (module docstring)"""
    r = bn_stats_reference(z)
    return float(r["mean"][channel].abs() / torch.sqrt(r["var"][channel])), float(r["b_rstd"][channel] / r["rstd"][channel])


def bn_operand_stats(z, eps=BN_EPS):
    """the f32 mean / rstd the forward and backward cases are given as operands: the fp64 statistics rounded once"""
    r = bn_stats_reference(z, eps=eps)
    return r["mean"].float(), r["rstd"].float()


def _sigmoid(u, d_u):
    sg = torch.sigmoid(u)
    rel_e = EPS * u.abs() + 2 * EXP_ULPS * EPS + d_u
    return sg, sg * (torch.sigmoid(-u) * rel_e + 2 * EPS)


def _u_of(xh, d_xh, gamma, beta):
    gx = gamma * xh
    u = gx + beta
    return u, gamma.abs() * d_xh + EPS * gx.abs() + EPS * u.abs()


def bf16_round64(v):
    """fp64 -> the nearest bf16 value (fp64) and the distance of v from the nearest rounding tie of bf16, with the size of that
    step: (q, tie_dist, step)"""
    q16 = v.float().to(torch.bfloat16)
    q = q16.double()
    bits = q16.view(torch.int16).to(torch.int32)
    away = (v.abs() >= q.abs())                                        # the second nearest neighbour lies further from zero
    nb = torch.where(away, bits + 1, bits - 1).to(torch.int16).view(torch.bfloat16).double()
    nb = torch.where(q == 0, torch.full_like(q, 2.0 ** -133) * torch.sign(v), nb)
    nb = torch.where(torch.isfinite(nb), nb, q)
    return q, (v - (q + nb) / 2).abs(), (nb - q).abs()


def bn_act_fwd_reference(z, mean, rstd, gamma, beta, res=None, act=1):
    """-> (a, B_a) in fp64 (module docstring); with a shortcut a = bf16(v) + res"""
    z, mean, rstd, gamma, beta = (t.double() for t in (z, mean, rstd, gamma, beta))
    xh = (z - mean) * rstd
    u, d_u = _u_of(xh, 2 * EPS * xh.abs(), gamma, beta)
    if act:
        sg, d_sg = _sigmoid(u, d_u)
        v = u * sg
        d_v = (u.abs() + d_u) * (sg + d_sg) - v.abs() + EPS * v.abs()
    else:
        v, d_v = u, d_u
    if res is None:
        return v, U * v.abs() + d_v
    q, tie_dist, step = bf16_round64(v)
    a = q + res.double()
    return a, U * a.abs() + EPS * a.abs() + d_v + torch.where(tie_dist <= 1.01 * d_v, step, torch.zeros_like(step))


def bn_act_bwd_reference(da, z, mean, rstd, gamma, beta, act=1, batch_stats=1):
    """-> dict in fp64: dz (T, C), dgamma, dbeta (C) and b_<name>"""
    d, z, mean, rstd, gamma, beta = (t.double() for t in (da, z, mean, rstd, gamma, beta))
    T, C = z.shape
    rel = _sum_rel(T, C)
    xh = (z - mean) * rstd
    d_xh = 2 * EPS * xh.abs()
    if act:
        u, d_u = _u_of(xh, d_xh, gamma, beta)
        sg, d_sg = _sigmoid(u, d_u)
        om = torch.sigmoid(-u)
        d_om = d_sg + EPS * om
        p = u * om
        d_p = (u.abs() + d_u) * (om + d_om) - p.abs() + EPS * p.abs()
        h = 1 + p
        d_h = d_p + EPS * h.abs()
        f = sg * h
        d_f = (sg + d_sg) * (h.abs() + d_h) - f.abs() + EPS * f.abs()
        gr = d * f
        d_gr = d.abs() * d_f + EPS * gr.abs()
    else:
        gr, d_gr = d, torch.zeros_like(d)
    gx = gr * xh
    d_gx = (gr.abs() + d_gr) * (xh.abs() + d_xh) - gx.abs() + EPS * gx.abs()
    dbeta, dgamma = gr.sum(0), gx.sum(0)
    e_dbeta = d_gr.sum(0) + rel * (gr.abs() + d_gr).sum(0)
    e_dgamma = d_gx.sum(0) + rel * (gx.abs() + d_gx).sum(0)
    if batch_stats:
        k1, k2 = dbeta / T, dgamma / T
        d_k1, d_k2 = e_dbeta / T + EPS * k1.abs(), e_dgamma / T + EPS * k2.abs()
    else:
        k1 = k2 = d_k1 = d_k2 = torch.zeros(C, dtype=torch.float64)
    xk = xh * k2
    d_xk = (xh.abs() + d_xh) * (k2.abs() + d_k2) - xk.abs() + EPS * xk.abs()
    t = gr - k1 - xk
    d_t = d_gr + d_k1 + d_xk + EPS * (gr - k1).abs() + EPS * t.abs()
    sc = gamma * rstd
    dz = sc * t
    return {"dz": dz, "b_dz": U * dz.abs() + sc.abs() * d_t + 2 * EPS * dz.abs(),
            "dgamma": dgamma, "b_dgamma": e_dgamma + EPS * dgamma.abs(), "dbeta": dbeta, "b_dbeta": e_dbeta + EPS * dbeta.abs()}


# ------------------------------------------------------------------------------------------------ A: f32 emulations
BN_MUTANTS = ("biased_running_var", "dz_without_k2", "silu_without_u_term", "drop_chunk_last_row", "drop_last_group",
              "res_before_rounding")


def emu_chan_reduce(v0, v1, mutant=None):
    """(T, C) f32 per-row terms -> their column sums (C) in double, in the order of chan_reduce_kernel + chunk_sums"""
    T, C = v0.shape
    chunks, rpc = chunks_for(T)
    out = []
    for v in (v0, v1):
        v = torch.cat([v.float(), torch.zeros(chunks * rpc - T, C)]).reshape(chunks, rpc, C).clone()
        if mutant == "drop_chunk_last_row":                               # `r < r1 - 1`
            for k in range(chunks):
                v[k, min(rpc, T - k * rpc) - 1] = 0
        if mutant == "drop_last_group":                                   # the thread of the last 8-channel group returns early
            v[..., C - 8:] = 0
        out.append(lane_chain(lane_chain(v, row_lanes(C)).double(), 32))
    return out


def emu_bn_stats(z, rm0=None, rv0=None, eps=BN_EPS, momentum=BN_MOMENTUM, mutant=None):
    """-> dict of f32: mean, rstd (and run_mean, run_var); bn_stats_final_kernel's double arithmetic in its order"""
    T = z.shape[0]
    zf = z.float()
    s, ss = emu_chan_reduce(zf, zf * zf, mutant)
    m = s / T
    var = (ss / T - m * m).clamp(min=0)
    out = {"mean": m.float(), "rstd": (1.0 / torch.sqrt(var + f32v(eps))).float()}
    if rm0 is not None:
        mom = f32v(momentum)
        unb = var * T / (T - 1) if T > 1 and mutant != "biased_running_var" else var
        out["run_mean"] = ((1.0 - mom) * rm0.double() + mom * m).float()
        out["run_var"] = ((1.0 - mom) * rv0.double() + mom * unb).float()
    return out


def _sig32(u):
    return 1.0 / (1.0 + torch.exp(-u))


def emu_bn_act_fwd(z, mean, rstd, gamma, beta, res=None, act=1, mutant=None):
    """-> a (T, C) bf16, bn_act_kernel<false> in its operation order"""
    u = gamma * ((z.float() - mean) * rstd) + beta
    v = u * _sig32(u) if act else u
    if res is not None:
        v = (v if mutant == "res_before_rounding" else bf(v).float()) + res.float()
    out = bf(v)
    if mutant == "drop_last_group":
        out[:, -8:] = 0
    return out


def emu_bn_act_bwd(da, z, mean, rstd, gamma, beta, act=1, batch_stats=1, mutant=None):
    """-> dz (T, C) bf16, dgamma, dbeta (C) f32"""
    T = z.shape[0]
    xh = (z.float() - mean) * rstd
    gr = da.float()
    if act:
        u = gamma * xh + beta
        sg = _sig32(u)
        gr = gr * (sg if mutant == "silu_without_u_term" else sg * (1.0 + u * (1.0 - sg)))
    s, sx = emu_chan_reduce(gr, gr * xh, mutant)
    k1 = (s / T).float() if batch_stats else torch.zeros_like(mean)
    k2 = (sx / T).float() if batch_stats else torch.zeros_like(mean)
    t = gr - k1 if mutant == "dz_without_k2" else gr - k1 - xh * k2
    dz = bf((gamma * rstd) * t)
    if mutant == "drop_last_group":
        dz[:, -8:] = 0
    return dz, sx.float(), s.float()


def bn_stats_exact(z, rm0, rv0, eps=BN_EPS, momentum=BN_MOMENTUM):
    """Integer z: the column sums are exact, so the outputs are bn_stats_final_kernel's formulas (lines 154-162) in IEEE double,
    in its order, rounded once -> mean, rstd, run_mean, run_var (f32 tensors)"""
    T = z.shape[0]
    s, ss = z.double().sum(0).numpy(), (z.double() ** 2).sum(0).numpy()
    eps, mom = np.float64(f32v(eps)), np.float64(f32v(momentum))
    m = s / np.float64(T)
    var = np.maximum(ss / np.float64(T) - m * m, 0.0)
    unb = var * np.float64(T) / np.float64(T - 1) if T > 1 else var
    rm = (1.0 - mom) * rm0.double().numpy() + mom * m
    rv = (1.0 - mom) * rv0.double().numpy() + mom * unb
    return tuple(torch.from_numpy(np.asarray(a, dtype=np.float64)).float() for a in (m, 1.0 / np.sqrt(var + eps), rm, rv))


# ------------------------------------------------------------------------------------------------ B: exact references
VIEW_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 1, 7)]                         # B, H, W (of the smaller grid)
POOL_SHAPES = [(1, 1), (2, 2), (3, 3), (5, 5), (3, 7), (7, 4)]          # the trainer's P5 grids: every window is clipped
POOL_PATTERNS = ("constant", "levels", "increasing")
IM2COL_SHAPES = [(1, 1), (5, 7), (6, 4)]
WDGRAD_SHAPES = [(3, 5), (16, 8), (40, 24)]                             # 9 * 40 * 24 = 8640 = 33 * 256 + 192
BLOB_PIXELS = (1, 255, 257)
SPPF_SHAPES = [(1, 1), (3, 7), (40, 40)]


def view_dst_dims(mode, H, W):
    return (2 * H, 2 * W) if mode in (2, 4) else ((H + 2, W + 2) if mode == 6 else (H, W))


def view_src_dims(mode, H, W):
    return (2 * H, 2 * W) if mode == 3 else (H, W)


@functools.lru_cache(maxsize=None)
def view_case(mode, B, H, W, C):
    g = torch.Generator().manual_seed(((mode * 7 + B) * 11 + H) * 13 + W + C)
    return {"src": int_tensor((B, *view_src_dims(mode, H, W), C), g), "dst0": int_tensor((B, *view_dst_dims(mode, H, W), C), g, -100, 100)}


def view_op_reference(mode, src, dst0, H, W, mutant=None):
    """yolo_train.hip:257-259 with plain indexing.  mutant zero_insert_odd: the values land on the odd positions"""
    dst = dst0.clone()
    DH, DW = view_dst_dims(mode, H, W)
    for y in range(DH):
        for x in range(DW):
            if mode == 0:
                dst[:, y, x] = src[:, y, x]
            elif mode == 1:
                dst[:, y, x] = dst0[:, y, x] + src[:, y, x]
            elif mode == 2:
                dst[:, y, x] = src[:, y // 2, x // 2]
            elif mode == 3:
                dst[:, y, x] = dst0[:, y, x] + src[:, 2 * y, 2 * x] + src[:, 2 * y, 2 * x + 1] + src[:, 2 * y + 1, 2 * x] + \
                    src[:, 2 * y + 1, 2 * x + 1]
            elif mode == 4:
                on = (y % 2 == 1 and x % 2 == 1) if mutant == "zero_insert_odd" else (y % 2 == 0 and x % 2 == 0)
                dst[:, y, x] = src[:, y // 2, x // 2] if on else 0
            elif mode == 5:
                dst[:, y, x] = 0
            else:
                dst[:, y, x] = src[:, y - 1, x - 1] if 1 <= y <= H and 1 <= x <= W else 0
    return dst


@functools.lru_cache(maxsize=None)
def pool_case(H, W, C, pattern, B=2):
    """x (B, H, W, C): constant (every window ties), three levels, or strictly increasing in scan order; dout in [-2, 2], din0 in
    [-3, 3]: at most 25 addends, every sum below 256"""
    g = torch.Generator().manual_seed((H * 17 + W) * 5 + C + POOL_PATTERNS.index(pattern))
    if pattern == "constant":
        x = torch.full((B, H, W, C), 3.0)
    elif pattern == "levels":
        x = torch.randint(0, 3, (B, H, W, C), generator=g).float()
    else:
        x = (torch.arange(H * W).float().view(1, H, W, 1) + torch.zeros(B, 1, 1, C)) * 0.5 - 4
    return {"x": x, "dout": int_tensor((B, H, W, C), g, -2, 2), "din0": int_tensor((B, H, W, C), g, -3, 3)}


def maxpool5_bwd_reference(x, dout, din0, mutant=None):
    """din0 + the adjoint of MaxPool2d(5, 1, 2): the window's FIRST maximum in scan order takes its gradient (mutant: the last)"""
    B, H, W, C = x.shape
    din = din0.clone()
    bi, ci = torch.arange(B).view(B, 1).expand(B, C), torch.arange(C).view(1, C).expand(B, C)
    for wy in range(H):
        for wx in range(W):
            best, by, bx = torch.full((B, C), -float("inf")), torch.zeros(B, C, dtype=torch.long), torch.zeros(B, C, dtype=torch.long)
            for yy in range(max(wy - 2, 0), min(wy + 3, H)):
                for xx in range(max(wx - 2, 0), min(wx + 3, W)):
                    v = x[:, yy, xx]
                    take = v >= best if mutant == "last_maximum" else v > best
                    best = torch.where(take, v, best)
                    by, bx = torch.where(take, torch.full_like(by, yy), by), torch.where(take, torch.full_like(bx, xx), bx)
            din[bi, by, bx, ci] += dout[:, wy, wx]
    return din


def im2col3_reference(x, stride, mutant=None):
    """x (B, Hin, Win, C) -> (B * Hout * Wout, 9 * C), Hout = (Hin - 1) // stride + 1 (k 3, pad 1); mutant: Hin // stride"""
    B, Hin, Win, C = x.shape
    Hout, Wout = ((Hin // stride, Win // stride) if mutant == "floor_out" else ((Hin - 1) // stride + 1, (Win - 1) // stride + 1))
    col = torch.zeros(B, Hout, Wout, 9, C)
    for oy in range(Hout):
        for ox in range(Wout):
            for tap in range(9):
                iy, ix = oy * stride + tap // 3 - 1, ox * stride + tap % 3 - 1
                if 0 <= iy < Hin and 0 <= ix < Win:
                    col[:, oy, ox, tap] = x[:, iy, ix]
    return col.reshape(B * Hout * Wout, 9 * C)


def weight_dgrad_reference(w):
    """w (Cout, taps, Cin) -> (Cin, taps, Cout) with the taps turned by 180 degrees"""
    Cout, taps, Cin = w.shape
    wd = torch.empty(Cin, taps, Cout, dtype=w.dtype)
    for tp in range(taps):
        wd[:, tp, :] = w[:, taps - 1 - tp, :].T
    return wd


def blob_case(pixels):
    """(pixels, 3) u8; 255 and 257 pixels hold all 256 byte values"""
    return ((torch.arange(pixels * 3) * 7 + pixels) % 256).to(torch.uint8).view(pixels, 3)


def blob_reference(img):
    """img (pixels, 3) u8 -> (pixels, 8) bf16: bf16(f32(v) * f32(1 / 255)), zero pad channels"""
    out = torch.zeros(img.shape[0], 8)
    out[:, :3] = img.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    return bf(out)


def _pool5(x):
    B, H, W, C = x.shape
    p = torch.full((B, H + 4, W + 4, C), -float("inf"))
    p[:, 2:H + 2, 2:W + 2] = x
    out = torch.full_like(x, -float("inf"))
    for dy in range(5):
        for dx in range(5):
            out = torch.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


def sppf_reference(x):
    """x (B, H, W, c) -> (B, H, W, 4 c): x and three chained clipped 5 x 5 maxima"""
    ys = [x]
    for _ in range(3):
        ys.append(_pool5(ys[-1]))
    return torch.cat(ys, -1)


# ------------------------------------------------------------------------------------------------ C: detection loss
RM, TOPK = 16, 10
CIOU_ERR, BRANCH_MARGIN, WEIGHT_FLOOR, SCORE_FLUSH = 1e-5, 1e-4, 1e-12, -120.0
GAINS = (7.5, 0.5, 1.5)
LOSS_OUTPUTS = ("loss", "dbox", "dcls")
# worst |f32 - f64| / (EPS * scale) of detect_loss_reference over LOSS_CASES, measured on the CPU (test_yolo_glue_reference_cpu.py
# asserts that a fresh measurement is not above these): the gate of the kernel is K = 8 * max(1, M)
LOSS_M = {"loss": 17.5, "dbox": 195.0, "dcls": 39.5}


def loss_k(name):
    return 8.0 * max(1.0, LOSS_M[name])


def loss_ws_layout(B, A, G):
    """float offsets of yv_detect_loss' workspace (yolo_loss.hip:366-377) -> dict name -> (offset in 4-byte words, words)"""
    bx = (A + 255) // 256
    out, o = {}, 0
    for name, n in (("pb", B * A * 4), ("iou", B * G * A), ("align", B * G * A), ("norm", B * A), ("pos", B * G * 2), ("part", bx * B * 3),
                    ("tss", 8), ("cnt", B * A), ("gsel", B * A), ("tgt", B * A)):
        out[name] = (o, n)
        o += n
    return out


def loss_ws_bytes(B, A, G):
    """yolo_loss.hip:340-345"""
    blocks = (A + 255) // 256 * B
    return (B * A * 4 + 2 * B * G * A + B * A + B * G * 2 + blocks * 3 + 8 + 3 * B * A) * 4 + 256


def anchors_of(S, dtype):
    """-> ax, ay (A) cell centres in grid units, stride (A), in the kernel's anchor order (anchor_of, yolo_loss.hip:45-51)"""
    ax, ay, st = [], [], []
    for s in (8, 16, 32):
        h = S // s
        i = torch.arange(h * h)
        ax.append((i % h).to(dtype) + 0.5)
        ay.append((i // h).to(dtype) + 0.5)
        st.append(torch.full((h * h,), float(s), dtype=dtype))
    return torch.cat(ax), torch.cat(ay), torch.cat(st)


def _ciou(p, t, dtype):
    """ciou_f (yolo_loss.hip:56-72) with its f32 constants; alpha carries no gradient"""
    eps, k4 = f32v(1e-7), f32v(0.40528473456935109)
    w1, h1, w2, h2 = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1] + eps, t[..., 2] - t[..., 0], t[..., 3] - t[..., 1] + eps
    iw = (torch.minimum(p[..., 2], t[..., 2]) - torch.maximum(p[..., 0], t[..., 0])).clamp(min=0)
    ih = (torch.minimum(p[..., 3], t[..., 3]) - torch.maximum(p[..., 1], t[..., 1])).clamp(min=0)
    inter = iw * ih
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    cw = torch.maximum(p[..., 2], t[..., 2]) - torch.minimum(p[..., 0], t[..., 0])
    ch = torch.maximum(p[..., 3], t[..., 3]) - torch.minimum(p[..., 1], t[..., 1])
    c2 = cw * cw + ch * ch + eps
    sx, sy = t[..., 0] + t[..., 2] - p[..., 0] - p[..., 2], t[..., 1] + t[..., 3] - p[..., 1] - p[..., 3]
    rho2 = (sx * sx + sy * sy) * 0.25
    da = torch.atan(w2 / h2) - torch.atan(w1 / h1)
    v = k4 * da * da
    alpha = (v / (v - iou + (1.0 + eps))).detach()
    return iou - (rho2 / c2 + v * alpha)


def detect_loss_reference(box, cls, gt_boxes, gt_labels, gt_counts, S, nc, dtype=torch.float64, gains=GAINS, ties="ascending",
                          claim="first", inside="gt", decisions=None):
    """The v8 detection loss of yolo_loss.hip restated from its operands in `dtype`.  box / cls: the three scales' (B h h, 64) /
    (B h h, ncp) logits; gt_boxes (B, G, 4) xyxy pixels, gt_labels (B, G), gt_counts (B).
    -> dict: loss (4: total * B, box, cls, dfl), dbox, dcls (lists like box / cls, columns [nc, ncp) of dcls zero), tgt (B, A) the
    box of every anchor or -1, weight (B, A), margins (dict), ok (bool: every margin of the module docstring holds).
    ties / claim / inside name the wrong kernels of the CPU test: top-k ties `descending`, claimant `last`, inside test `ge`.
    decisions: take tgt from another evaluation (the f32 evaluation for K is given the fp64 decisions: the margins make that the
    same thing, and the constants then measure arithmetic only)."""
    B, G = gt_boxes.shape[:2]
    ncp = cls[0].shape[1]
    ax, ay, st = anchors_of(S, dtype)
    A = ax.numel()
    hs = [S // 8, S // 16, S // 32]
    boxl = [b.to(dtype).clone().requires_grad_(True) for b in box]
    clsl = [c.to(dtype).clone().requires_grad_(True) for c in cls]
    bx = torch.cat([b.view(B, h * h, 64) for b, h in zip(boxl, hs)], 1)                       # (B, A, 64)
    cx = torch.cat([c.view(B, h * h, ncp) for c, h in zip(clsl, hs)], 1)[..., :nc]            # (B, A, nc)
    gtb = gt_boxes.to(dtype)
    lab = gt_labels.long().clamp(0, nc - 1)
    valid = torch.arange(G)[None] < gt_counts.long()[:, None]                                 # (B, G)
    proj = torch.arange(RM, dtype=dtype)
    prob = bx.view(B, A, 4, RM).softmax(-1)
    dist = (prob * proj).sum(-1)                                                              # (B, A, 4)
    pb = torch.stack([ax - dist[..., 0], ay - dist[..., 1], ax + dist[..., 2], ay + dist[..., 3]], -1)      # grid units
    with torch.no_grad():
        px, py = ax * st, ay * st
        pbp = pb * st[None, :, None]
        g4 = gtb[:, :, None, :]                                                               # (B, G, 1, 4)
        dm = torch.minimum(torch.minimum(px - g4[..., 0], py - g4[..., 1]), torch.minimum(g4[..., 2] - px, g4[..., 3] - py))     # (B, G, A)
        ins = ((dm >= 0) if inside == "ge" else (dm > f32v(1e-9))) & valid[..., None]
        ciou_m = _ciou(g4.expand(B, G, A, 4), pbp[:, None].expand(B, G, A, 4), dtype)
        xl = cx.gather(2, lab[:, None, :].expand(B, A, G)).permute(0, 2, 1)                   # (B, G, A) logit of the box's class
        score = torch.where(xl <= SCORE_FLUSH, torch.zeros_like(xl), torch.sigmoid(xl))
        iou = torch.where(ins, ciou_m.clamp(min=0), torch.zeros_like(ciou_m))
        align = torch.where(ins, torch.sqrt(score) * iou ** 6, torch.zeros_like(iou))
        exact0 = ins & ((xl <= SCORE_FLUSH) | (ciou_m <= -CIOU_ERR))                          # metric 0 on both sides by construction
        margins = {"flush": float(((xl > SCORE_FLUSH) & (xl < -80.0) & ins).sum())}           # scores in f32's denormal range: none
        # ---- top-k of every box among the anchors inside it
        metric = torch.where(ins, align, torch.full_like(align, -1.0))
        if ties == "descending":
            order = (A - 1) - metric.flip(-1).sort(dim=-1, descending=True, stable=True).indices
        else:
            order = metric.sort(dim=-1, descending=True, stable=True).indices
        k = min(TOPK, A)
        chosen = torch.zeros(B, G, A, dtype=torch.bool)
        chosen.scatter_(-1, order[..., :k], True)
        chosen &= ins
        up = torch.sqrt(score) * (iou + CIOU_ERR) ** 6 * (1 + 1e-5)
        lo = torch.sqrt(score) * (iou - CIOU_ERR).clamp(min=0) ** 6 * (1 - 1e-5)
        cp, rest = chosen & ~exact0, ins & ~chosen & ~exact0                                   # chosen / left out, not exact zeros
        cz = chosen & exact0
        inf = torch.full_like(lo, float("inf"))
        lo_c = torch.where(cp, lo, inf).amin(-1)                                              # (B, G)
        up_r = torch.where(rest, up, -inf).amax(-1)
        topk_ok = (lo_c > up_r) & (torch.where(cp, lo, inf).amin(-1) > 0) & ~(cz.any(-1) & rest.any(-1))
        margins["topk"] = bool(topk_ok.all())
        both = torch.isfinite(lo_c) & torch.isfinite(up_r)                                    # relative gap between the 10th and the 11th
        margins["topk_gap"] = float(((lo_c - up_r) / lo_c.clamp(min=1e-300))[both].min()) if bool(both.any()) else float("inf")
        # ---- one box per anchor
        cnt = chosen.sum(1)                                                                   # (B, A)
        iou_v = torch.where(valid[..., None], iou, torch.full_like(iou, -1.0))
        if claim == "last":
            best = (G - 1) - iou_v.flip(1).argmax(1)
        else:
            best = iou_v.argmax(1)
        single = chosen.float().argmax(1)
        tgt = torch.where(cnt > 1, best, torch.where(cnt == 1, single, torch.full_like(single, -1)))
        top2 = iou_v.topk(min(2, G), dim=1)
        if G > 1:
            box_of = lambda j: gtb.gather(1, top2.indices[:, j][..., None].expand(B, A, 4))
            same_box = (box_of(0) == box_of(1)).all(-1)
            both0 = exact0.gather(1, top2.indices).all(1) | ((top2.values[:, 0] == 0) & ~(ins & ~exact0 & (iou == 0)).any(1))
            second_valid = top2.values[:, 1] >= 0
            claim_ok = ~(cnt > 1) | ~second_valid | (top2.values[:, 0] - top2.values[:, 1] > 2 * CIOU_ERR) | same_box | both0
            margins["claim"] = bool(claim_ok.all())
        else:
            margins["claim"] = True
        if decisions is not None:
            tgt = decisions
        fg = tgt >= 0
        tsafe = tgt.clamp(min=0)
        pos = _box_onehot(tsafe, G) & fg[:, None, :]                                             # (B, G, A)
        pos_align = torch.where(pos, align, torch.zeros_like(align)).amax(-1)                 # (B, G)
        pos_iou = torch.where(pos, iou, torch.zeros_like(iou)).amax(-1)
        a_t = align.gather(1, tsafe[:, None, :])[:, 0]                                        # (B, A)
        weight = torch.where(fg, a_t * pos_iou.gather(1, tsafe) / (pos_align.gather(1, tsafe) + f32v(1e-9)), torch.zeros_like(a_t))
        tss = weight.sum().clamp(min=1.0)
        tlab = lab.gather(1, tsafe)
        tscore = torch.zeros(B, A, nc, dtype=dtype)
        tscore.scatter_(2, tlab[..., None], weight[..., None])
        tb = gtb.gather(1, tsafe[..., None].expand(B, A, 4)) / st[None, :, None]              # grid units
        wpos = fg & (weight > 0)
        margins["weight"] = float(weight[wpos].min()) if bool(wpos.any()) else float("inf")
        tl4 = torch.stack([ax - tb[..., 0], ay - tb[..., 1], tb[..., 2] - ax, tb[..., 3] - ay], -1)
        tmax = float(torch.tensor(float(RM - 1), dtype=torch.float32) - torch.tensor(0.01, dtype=torch.float32))
        tt = tl4.clamp(0, tmax)
        tl = tt.floor().long()
        wl = (tl + 1).to(dtype) - tt
        if bool(wpos.any()):
            p_, t_ = pb[wpos], tb[wpos]
            gaps = torch.cat([(p_ - t_).abs().reshape(-1),
                              (torch.minimum(p_[:, 2], t_[:, 2]) - torch.maximum(p_[:, 0], t_[:, 0])).abs(),
                              (torch.minimum(p_[:, 3], t_[:, 3]) - torch.maximum(p_[:, 1], t_[:, 1])).abs()])
            margins["branch"] = float(gaps.min())
            raw = tl4[wpos]
            frac = (raw - raw.round()).abs()
            margins["dfl_integer"] = float(frac[frac > 0].min()) if bool((frac > 0).any()) else float("inf")
            margins["dfl_clamped"] = int(((raw > tmax) | (raw < 0)).sum())
        else:
            margins.update(branch=float("inf"), dfl_integer=float("inf"), dfl_clamped=0)
    bce = cx.clamp(min=0) - cx * tscore + torch.log1p(torch.exp(-cx.abs()))
    s_cls = bce.sum()
    ci = _ciou(pb, tb, dtype)
    s_box = (torch.where(fg, (1.0 - ci) * weight, torch.zeros_like(ci))).sum()
    logp = torch.log_softmax(bx.view(B, A, 4, RM), -1)
    dfl = -(logp.gather(-1, tl[..., None])[..., 0] * wl + logp.gather(-1, (tl + 1)[..., None])[..., 0] * (1.0 - wl))
    s_dfl = (torch.where(fg[..., None], dfl * 0.25 * weight[..., None], torch.zeros_like(dfl))).sum()
    l_box, l_cls, l_dfl = s_box / tss, s_cls / tss, s_dfl / tss
    total = (gains[0] * l_box + gains[1] * l_cls + gains[2] * l_dfl) * B
    total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    dcls = []
    for c in clsl:
        gq = zero(c).clone()
        gq[:, nc:] = 0
        dcls.append(gq)
    ok = margins["topk"] and margins["claim"] and margins["flush"] == 0 and margins["branch"] >= BRANCH_MARGIN and \
        margins["weight"] >= WEIGHT_FLOOR
    return {"loss": torch.stack([total.detach(), l_box.detach(), l_cls.detach(), l_dfl.detach()]), "dbox": [zero(b) for b in boxl],
            "dcls": dcls, "tgt": tgt, "weight": weight, "margins": margins, "ok": bool(ok), "inside": ins, "chosen": chosen}


def _box_onehot(idx, G):
    """(B, A) -> (B, G, A) bool"""
    return torch.arange(G)[None, :, None] == idx[:, None, :]


# name -> S, B, G, counts, nc, ncp, kind
LOSS_CASES = {
    "s32": (32, 2, 1, [1, 1], 1, 8, "rand"),                  # A = 21: one partly filled workgroup; fewer than ten anchors inside
    "s64": (64, 2, 6, [6, 0], 5, 8, "labels"),                # an image without a box; labels -3 and nc + 2
    "s160": (160, 2, 6, [6, 3], 80, 80, "big"),               # ncp = nc = 80; a box wider than 15 stride-8 cells; logits at +-30
    "empty": (64, 2, 1, [0, 0], 5, 8, "rand"),                # no box at all: the normaliser clamps to 1, dbox is zero
    "s640": (640, 1, 6, [6], 5, 8, "rand"),                   # A = 8400: the strided loops
    "metric0": (64, 1, 1, [1], 5, 8, "metric0"),              # class logit -200 everywhere: every metric 0, the ten lowest indices win
    "twins": (64, 1, 6, [3], 5, 8, "twins"),                  # two identical boxes: the lower index takes every shared anchor
    "edges": (64, 1, 1, [1], 5, 8, "edges"),                  # edges at multiples of 4 through stride-8 centres: those are outside
    "small": (64, 1, 6, [2], 5, 8, "small"),                  # one anchor inside, and none
}


def _lattice(t):
    return (t * 4).round() / 4


def _loss_operands(name, seed):
    S, B, G, counts, nc, ncp, kind = LOSS_CASES[name]
    g = torch.Generator().manual_seed(seed)
    box, cls = [], []
    for h in (S // 8, S // 16, S // 32):
        b = torch.randn(B * h * h, 64, generator=g) * 1.5
        c = torch.full((B * h * h, ncp), float("nan"))                   # columns [nc, ncp) are not read
        c[:, :nc] = torch.randn(B * h * h, nc, generator=g) * 1.5 - 1.0
        if kind == "big":                                                # logits at +-30, box and class (nc = ncp: c is dense)
            b.view(-1)[::97] = 30.0
            b.view(-1)[5::89] = -30.0
            c.view(-1)[::83] = 30.0
            c.view(-1)[7::79] = -30.0
        box.append(b)
        cls.append(c)
    ctr = torch.rand(B, G, 2, generator=g) * S
    wh = torch.rand(B, G, 2, generator=g) * S * 0.45 + 10.0
    gtb = _lattice(torch.cat([(ctr - wh / 2).clamp(0, S), (ctr + wh / 2).clamp(0, S)], -1))
    gtl = torch.randint(0, nc, (B, G), generator=g, dtype=torch.int32)
    if kind == "labels":
        gtl[0, 1], gtl[0, 2] = -3, nc + 2
    if kind == "big":
        gtb[0, 0] = torch.tensor([4.0, 10.25, 156.0, 150.5])             # 19 stride-8 cells wide
    if kind == "metric0":
        gtb[0, 0] = torch.tensor([9.0, 9.0, 55.0, 47.0])
        for c in cls:
            c[:, int(gtl[0, 0])] = -200.0
    if kind == "twins":
        gtb[0, 0] = torch.tensor([8.25, 6.0, 50.0, 44.5])                # more than ten anchors inside
        gtb[0, 1] = gtb[0, 0]
        gtl[0, 1] = gtl[0, 0]
    if kind == "edges":
        gtb[0, 0] = torch.tensor([4.0, 4.0, 36.0, 28.0])
    if kind == "small":
        gtb[0, 0] = torch.tensor([17.0, 17.0, 23.0, 23.0])               # the stride-8 centre (20, 20) only
        gtb[0, 1] = torch.tensor([40.25, 40.25, 41.25, 41.25])           # between centres: no anchor inside
    if name == "s32":
        gtb[0, 0] = torch.tensor([2.0, 2.0, 30.0, 22.0])                 # 4 x 3 stride-8 centres, 2 x 1 stride-16, the stride-32 one
        gtb[1, 0] = torch.tensor([9.0, 9.0, 15.0, 15.0])                 # one stride-8 centre
    return box, cls, gtb, gtl, torch.tensor(counts, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """-> dict: box, cls (lists), gtb, gtl, cnt, S, nc, ncp, ref (detect_loss_reference in fp64), seed.  Seeds are tried in order
    until every margin of the module docstring holds (asserted)."""
    S, B, G, counts, nc, ncp, kind = LOSS_CASES[name]
    for seed in range(1000 * (sorted(LOSS_CASES).index(name) + 1), 1000 * (sorted(LOSS_CASES).index(name) + 1) + 200):
        box, cls, gtb, gtl, cnt = _loss_operands(name, seed)
        assert bool((gtb * 4 == (gtb * 4).round()).all()) and float(gtb.max()) <= 1000       # the 1/4-pixel lattice
        ref = detect_loss_reference(box, cls, gtb, gtl, cnt, S, nc)
        if ref["ok"]:
            return {"box": box, "cls": cls, "gtb": gtb, "gtl": gtl, "cnt": cnt, "S": S, "B": B, "G": G, "nc": nc, "ncp": ncp, "ref": ref,
                    "seed": seed, "A": ref["tgt"].shape[1]}
    raise AssertionError(f"{name}: no seed satisfies the margins: {ref['margins']}")


ORACLE_CASES = [(3, 160, 6, [4, 0, 6], 0), (2, 320, 12, [12, 7], 1), (2, 96, 3, [0, 0], 2), (4, 160, 5, [1, 5, 2, 3], 3)]


def oracle_case(B, S, G, counts, seed, nc=5, ncp=8):
    """the operands of test_gpu_yolo_train.py::test_detect_loss_vs_oracle (same draws) -> (outs for oracle.detection_loss, box, cls,
    gtb, gtl, cnt): on these the f32 evaluation of detect_loss_reference is compared with the oracle"""
    g = torch.Generator().manual_seed(seed)
    outs, box, cls = [], [], []
    for h in (S // 8, S // 16, S // 32):
        b = torch.randn(B, 64, h, h, generator=g) * 1.5
        c = torch.randn(B, nc, h, h, generator=g) * 1.5 - 1.0
        outs.append((b.clone().requires_grad_(True), c.clone().requires_grad_(True)))
        box.append(b.permute(0, 2, 3, 1).reshape(-1, 64).contiguous())
        cp = torch.zeros(B * h * h, ncp)
        cp[:, :nc] = c.permute(0, 2, 3, 1).reshape(-1, nc)
        cls.append(cp)
    ctr = torch.rand(B, G, 2, generator=g) * S
    wh = torch.rand(B, G, 2, generator=g) * S * 0.45 + 2.0
    wh[:, 0] = 6.0
    gtb = torch.cat([(ctr - wh / 2).clamp(0, S), (ctr + wh / 2).clamp(0, S)], -1)
    gtl = torch.randint(0, nc, (B, G), generator=g)
    return outs, box, cls, gtb, gtl.to(torch.int32), torch.tensor(counts, dtype=torch.int32)


def loss_scale(ref_rows):
    """|ref| + max|ref| over the element's row, for a (rows, cols) reference"""
    return ref_rows.abs() + ref_rows.abs().amax(-1, keepdim=True)


def loss_ratios(got, ref):
    """got / ref: dicts with loss (4), dbox, dcls (lists) -> {output: worst |got - ref| / (EPS * scale)}; 0 / 0 counts as 0"""
    rl = ref["loss"].reshape(-1, 1).double()
    out = {"loss": worst(got["loss"].reshape(-1, 1), rl, EPS * loss_scale(rl))[0]}
    for name in ("dbox", "dcls"):
        out[name] = max(worst(g, r.double(), EPS * loss_scale(r.double()))[0] for g, r in zip(got[name], ref[name]))
    return out


def measure_loss_m():
    """-> {output: worst |f32 - f64| / (EPS * scale) over LOSS_CASES} of this file's formulas evaluated in f32 with torch"""
    m = {k: 0.0 for k in LOSS_OUTPUTS}
    for name in LOSS_CASES:
        c = loss_case(name)
        f32 = detect_loss_reference(c["box"], c["cls"], c["gtb"], c["gtl"], c["cnt"], c["S"], c["nc"], dtype=torch.float32,
                                    decisions=c["ref"]["tgt"])
        for k, v in loss_ratios(f32, c["ref"]).items():
            m[k] = max(m[k], v)
    return m
